// vrc_api.cpp -- C-ABI host layer of libvrc.so (see include/vrc.h).
//
// Plays the role of src/CLCaster.cpp in the reference: owns the device
// buffers (its named buffer_map, :855-944), the settings buffer (:1029-1109),
// validation (:157-206) and the per-frame launch (:224-228, 946-987) -- with
// HIP streams/events on MI355X instead of an OpenCL queue + GL interop.
//
// A handle drives one GPU.  A GROUP handle (vrc_create_group) is rank 0 of a set of handles, one per GPU, that share
// one host thread: every assign_* / setting call is replicated, the octree is uploaded once and fanned out
// device-to-device, each rank owns only its row bands of the ray table / frame (vrc_set_row_slice), vrc_compute
// launches all ranks and returns when all are done, and the read-back calls gather every rank's rows into the
// caller's frame.  No collective anywhere.  (The calls that read the resident scene: vrc_query.cpp; the calls that
// change it: vrc_scene_edit.cpp.)
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "vrc_host.hpp"

#ifdef VRC_INDEX_AUDIT
namespace vrc {
#define VRC_AUDIT_DECLARE(name) hipError_t audit_publish_##name(const unsigned long long *extent_plus_1); hipError_t audit_collect_##name(audit::Stat *out, unsigned long long *extent_plus_1, int clear);
VRC_AUDIT_DECLARE(raycast) VRC_AUDIT_DECLARE(jump) VRC_AUDIT_DECLARE(boxes) VRC_AUDIT_DECLARE(query) VRC_AUDIT_DECLARE(boxq) VRC_AUDIT_DECLARE(sweep) VRC_AUDIT_DECLARE(read) VRC_AUDIT_DECLARE(edit) VRC_AUDIT_DECLARE(compact) VRC_AUDIT_DECLARE(region) VRC_AUDIT_DECLARE(faces)
#undef VRC_AUDIT_DECLARE
}  // namespace vrc
#endif

// (the helpers vrc_host.hpp declares are defined in its namespace, everything else of this file in the anonymous one)
int vrc_host::fail(vrc_caster *h, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->error = buf;
    return code;
}

void vrc_host::release_boxes(vrc_tree *t) {
    release(t->d_boxes); release(t->d_box_aux); release(t->d_box_child); release(t->d_box_desc); release(t->d_box_pos);
    t->boxes.built = BoxKey{}; t->box_records = 0; t->box_levels = 0;
}

void vrc_host::bind_attachments(const vrc_tree *t, const uint32_t *&attach_lookup, const uint64_t *&attachments) {
    attach_lookup = (t->d_attach_lookup && t->d_attach) ? t->d_attach_lookup : nullptr;
    attachments = attach_lookup ? t->d_attach : nullptr;
}

namespace {

// vrc_cast_rays', vrc_box_intersection's, vrc_sweep_boxes', the voxel reads', the face extraction's and the voxel edits' staging and scratch buffers (the caller's device is left
// as it was)
void release_query_staging(vrc_caster *h) {
    if (!h->d_query_rays && !h->d_query_out && !h->d_box_in && !h->d_box_vox && !h->d_box_plan && !h->d_box_items && !h->d_box_temp &&
        !h->d_sweep_in && !h->d_sweep_rec && !h->d_read_in && !h->d_read_out && !h->d_edit_in && !h->d_edit_keys && !h->d_edit_counters &&
        !h->d_edit_temp && !h->d_edit_levels && !h->d_edit_rec_masks && !h->d_region_in && !h->d_region_counts && !h->d_face_items) return;
    {
        DeviceRestore restore;
        (void)hipSetDevice(h->device);
        release(h->d_query_rays); release(h->d_query_out);
        h->query_capacity = 0;
        release(h->d_box_in); release(h->d_box_rec); release(h->d_box_cnt); release(h->d_box_vox);
        release(h->d_box_plan); release(h->d_box_scan); release(h->d_box_corner); release(h->d_box_items); release(h->d_box_temp);
        h->box_io_capacity = 0; h->box_vox_bytes = 0; h->box_capacity = 0; h->box_item_capacity = 0; h->box_temp_bytes = 0;
        release(h->d_sweep_in); release(h->d_sweep_out); release(h->d_sweep_rec); release(h->d_sweep_vox); release(h->d_sweep_cnt); release(h->d_sweep_scan);
        h->sweep_io_capacity = 0; h->sweep_capacity = 0;
        release(h->d_read_in); release(h->d_read_out);
        h->read_in_capacity = 0; h->read_out_bytes = 0;
        release(h->d_face_items);
        h->face_item_capacity = 0;
        release(h->d_edit_in); release(h->d_edit_keys); release(h->d_edit_unique); release(h->d_edit_order); release(h->d_edit_counts);
        release(h->d_edit_counters); release(h->d_edit_temp); release(h->d_edit_levels); release(h->d_edit_rec_masks); release(h->d_edit_rec_child);
        h->edit_in_capacity = 0; h->edit_capacity = 0; h->edit_temp_bytes = 0; h->edit_level_capacity = 0; h->edit_rec_capacity = 0;
        release(h->d_region_in); release(h->d_region_counts);
        h->region_in_bytes = 0; h->region_capacity = 0;
    }
    (void)hipGetLastError();
}

// what create_viewport allocates and a frame adds to it
void release_viewport_buffers(vrc_caster *h) {
    release(h->d_viewport); release(h->d_image); release(h->d_hits); release(h->d_rgba8); release(h->d_jump_cache); release(h->d_jump_slots);
    h->jump_slot_count = 0;
}

// the handle lets go of its tree; the arrays, the table and the boxes are freed with the last handle that holds them
void release_tree(vrc_caster *h) {
    h->tree.reset();
    h->owns_desc = true;
    h->validated = false;
}
// ... and so does its whole group: the peers first (ranks sharing rank 0's arrays must let go before rank 0 does).  Called BEFORE a
// new tree is built or uploaded: the old one must be gone by then (trees of BASELINE configs[4]'s size do not fit twice), and a
// new tree never inherits the old one's materials
void drop_trees(vrc_caster *h) {
    for (vrc_caster *q : h->peers) release_tree(q);
    release_tree(h);
}
// a fresh tree on this GPU, held by nobody yet: the caller fills it and attaches it only once it is complete (install_tree), so a
// step that fails on the way just lets it go
std::shared_ptr<vrc_tree> new_tree(int device, uint64_t *d_desc = nullptr, uint64_t n_desc = 0) {
    std::shared_ptr<vrc_tree> t = std::make_shared<vrc_tree>();
    t->device = device; t->d_desc = d_desc; t->n_desc = n_desc;
    return t;
}

#ifdef VRC_INDEX_AUDIT
// the index-audit build: the extents published last and the table of every .hip file they are published to (vrc_host.hpp)
struct AuditTu { hipError_t (*publish)(const unsigned long long *); hipError_t (*collect)(vrc::audit::Stat *, unsigned long long *, int); };
const AuditTu kAuditTus[] = {
    {vrc::audit_publish_raycast, vrc::audit_collect_raycast}, {vrc::audit_publish_jump, vrc::audit_collect_jump},
    {vrc::audit_publish_boxes, vrc::audit_collect_boxes},     {vrc::audit_publish_query, vrc::audit_collect_query},
    {vrc::audit_publish_boxq, vrc::audit_collect_boxq},       {vrc::audit_publish_sweep, vrc::audit_collect_sweep},
    {vrc::audit_publish_read, vrc::audit_collect_read},       {vrc::audit_publish_edit, vrc::audit_collect_edit},
    {vrc::audit_publish_compact, vrc::audit_collect_compact}, {vrc::audit_publish_region, vrc::audit_collect_region},
    {vrc::audit_publish_faces, vrc::audit_collect_faces},
};
}  // namespace
unsigned long long vrc_host::g_audit_shrink[vrc::audit::kArrayCount];
unsigned long long vrc_host::g_audit_current[vrc::audit::kArrayCount];
hipError_t vrc_host::audit_publish(const AuditExtents &x) {
    hipError_t e = hipDeviceSynchronize();
    for (const AuditTu &tu : kAuditTus)
        if (e == hipSuccess) e = tu.publish(x.e1);
    memcpy(g_audit_current, x.e1, sizeof(g_audit_current));
    return e;
}
void vrc_host::audit_tree(AuditExtents &x, const vrc_tree *t) {
    using namespace vrc::audit;
    x.set(kDescriptors, t->n_desc); x.set(kFarSlots, t->n_desc);
    const bool attach = t->d_attach_lookup && t->d_attach;
    x.set(kAttachLookup, attach ? t->n_desc : 0);
    x.set(kAttachments, attach ? std::max<uint64_t>(t->n_attach, 1) : 0);
    x.set(kCoarse, t->d_coarse ? 1ULL << (3 * t->coarse.built.log2) : 0);
    x.set(kBoxAux, t->d_box_aux ? 1ULL << (3 * t->coarse.built.log2) : 0);
    x.set(kBoxes, t->d_boxes ? 8 * t->box_records : 0);
    x.set(kBoxChild, t->d_box_child ? t->box_records : 0);
}
namespace {
#endif

int prepare_one(vrc_caster *h);           // (below, beside the launch path that shares derive_from_tree with it)

int find_setting(const vrc_caster *h, const char *name) {
    for (size_t i = 0; i < h->settings.size(); i++)
        if (h->settings[i].name == name) return (int)i;
    return -1;
}

// coarse_log2 / empty_boxes / empty_box_records / empty_box_levels set (again) by the host: a build that failed before -- a transient out-of-memory, a level asked too
// large -- is tried again by the next vrc_prepare / frame
void retry_derived(vrc_caster *h, const char *name) {
    if (!h->tree || (strcmp(name, "coarse_log2") != 0 && strcmp(name, "empty_boxes") != 0 && strcmp(name, "empty_box_records") != 0 &&
                     strcmp(name, "empty_box_levels") != 0)) return;
    std::lock_guard<std::mutex> lock(h->tree->guard);
    h->tree->coarse.gave_up = h->tree->boxes.gave_up = false;
}

}  // namespace

int64_t vrc_host::setting_or(const vrc_caster *h, const char *name, int64_t dflt) {
    int i = find_setting(h, name);
    return i < 0 ? dflt : h->settings[i].value;
}

int vrc_host::set_setting(vrc_caster *h, const char *name, const char *define, int64_t value) {
    retry_derived(h, name);
    int i = find_setting(h, name);
    if (i >= 0) { h->settings[i].value = value; return VRC_OK; }
    if (h->settings.size() >= 64) return fail(h, VRC_ERR_LIMIT, "settings buffer is full (64 slots)");
    h->settings.push_back({name, define ? define : "", value});
    return VRC_OK;
}

int vrc_host::log2_exact(int64_t v) {
    if (v < 2 || (v & (v - 1))) return -1;
    int n = 0;
    while ((1LL << n) < v) n++;
    return n;
}

namespace {

void drain_events(vrc_caster *h) {
    for (auto &p : h->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { h->timed_ms += ms; h->timed_launches++; }
        h->pool.push_back(p);
    }
    h->pending.clear();
}

// The rows a handle renders, as runs: image rows [y0, y0 + n) live at buffer rows [b0, b0 + n).
struct RowRun { int32_t y0, n, b0; };
std::vector<RowRun> row_runs(const vrc_caster *h, bool buffer_sliced) {
    std::vector<RowRun> runs;
    int32_t b0 = 0;
    for (int32_t y = h->tile_rank * h->band_rows; y < h->height; y += h->tile_world * h->band_rows) {
        const int32_t n = std::min(h->band_rows, h->height - y);
        runs.push_back({y, n, buffer_sliced ? b0 : y});
        b0 += n;
    }
    return runs;
}
int32_t local_row_count(const vrc_caster *h) {
    int32_t rows = 0;
    for (const RowRun &r : row_runs(h, true)) rows += r.n;
    return rows;
}

// one row of the reference's ray table (CLCaster.cpp:233-275): base ray (-800, x, y) slewed by the literal 1.57 about
// Y in double, then normalised in float (util.hpp:64-73)
void reference_table_row(int32_t width, int32_t height, int32_t row, float *out) {
    const double s157 = std::sin(1.57), c157 = std::cos(1.57);
    const int y = row - height / 2;
    for (int x = -width / 2; x < width / 2; x++) {
        const float bx = -800.0f, by = (float)x, bz = (float)y;
        const float rx = (float)((double)bz * s157 + (double)bx * c157);
        const float ry = by;
        const float rz = (float)((double)bz * c157 - (double)bx * s157);
        const float len = std::sqrt(rx * rx + ry * ry + rz * rz);
        float *t = out + 4 * (size_t)(x + width / 2);
        t[0] = rx / len; t[1] = ry / len; t[2] = rz / len; t[3] = 0.0f;
    }
}

// allocate the viewport buffers (all rows, or this rank's rows when sliced) and upload the ray table run by run;
// table == nullptr: the reference's own table
int install_viewport(vrc_caster *h, int32_t width, int32_t height, const float *table) {
    HIP_TRY(h, hipSetDevice(h->device));
    release_viewport_buffers(h);
    h->width = width; h->height = height;
    h->buffer_rows = h->sliced ? local_row_count(h) : height;
    h->validated = false;
    const size_t npix = (size_t)width * (size_t)std::max(h->buffer_rows, 1);
    HIP_TRY(h, hipMalloc((void **)&h->d_viewport, 16 * npix));
    HIP_TRY(h, hipMalloc((void **)&h->d_image, 16 * npix));
    std::vector<RowRun> runs = h->sliced ? row_runs(h, true) : std::vector<RowRun>{{0, height, 0}};
    std::vector<float> stage;
    const int32_t chunk = 64;                                     // rows per host staging buffer
    for (const RowRun &r : runs)
        for (int32_t o = 0; o < r.n; o += chunk) {
            const int32_t n = std::min(chunk, r.n - o);
            const float *src = table ? table + 4 * (size_t)width * (size_t)(r.y0 + o) : nullptr;
            if (!table) {
                // the reference's loops run x, y over [-w/2, w/2) x [-h/2, h/2): with an odd size the last column / row
                // of its (zero-initialised) table is never written (CLCaster.cpp:242-275)
                stage.assign(4 * (size_t)width * n, 0.0f);
                for (int32_t k = 0; k < n; k++)
                    if (r.y0 + o + k < 2 * (height / 2))
                        reference_table_row(width, height, r.y0 + o + k, stage.data() + 4 * (size_t)width * k);
                src = stage.data();
            }
            HIP_TRY(h, hipMemcpy(h->d_viewport + 4 * (size_t)width * (size_t)(r.b0 + o), src, 16 * (size_t)width * n, hipMemcpyHostToDevice));
        }
    // the image starts as RGBA8 (255,255,255,100)  (CLCaster.cpp:280-286)
#ifdef VRC_INDEX_AUDIT
    { AuditExtents x; x.set(vrc::audit::kImage, npix); VRC_AUDIT_PUBLISH(h, x); }
#endif
    HIP_TRY(h, vrc::launch_fill_image(h->d_image, npix, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return VRC_OK;
}

// the per-ray Euclid tables of the exact closed-form jumps (exact_jump.hpp): kJumpTableDwordsPerLane dwords per lane of a
// workgroup SLOT of wg_tiles tiles.  Only resident workgroups hold a slot (the kernel takes and returns them), so the buffer is sized
// for the chip, not for the frame: 8 x 256 slots of 12 KB with 4-tile workgroups, 8 x 1024 of 3 KB with single-tile ones.
int ensure_jump_cache(vrc_caster *h, int nblocks, int wg_tiles) {
    // an eighth of the slots per XCD, each eighth at least as large as the number of workgroups one XCD can hold at a time: its
    // CUs x the workgroups of this size a CU holds at most (MI355X: 32 x 8 = kJumpSlotsPerXcd 256-thread blocks, 32 x 32 waves; a
    // larger part gets larger eighths, and the kernel's slot search is bounded in any case)
    int cus = 0, threads_per_cu = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) cus = 256;
    if (hipDeviceGetAttribute(&threads_per_cu, hipDeviceAttributeMaxThreadsPerMultiProcessor, h->device) != hipSuccess) threads_per_cu = 2048;
    (void)hipGetLastError();
    const int wg_threads = 64 * wg_tiles;
    const int per_xcd = std::max(vrc::kJumpSlotsPerXcd, ((cus + 7) / 8) * std::max(1, threads_per_cu / wg_threads));
    const int slots = 8 * std::max(1, std::min(nblocks, per_xcd));
    if (h->d_jump_cache && h->jump_slot_count >= slots && h->jump_slot_threads >= wg_threads) return VRC_OK;
    release(h->d_jump_cache); release(h->d_jump_slots);
    h->jump_slot_count = 0;
    HIP_TRY(h, hipMalloc((void **)&h->d_jump_cache, (size_t)slots * wg_threads * vrc::kJumpTableDwordsPerLane * sizeof(uint32_t)));
    HIP_TRY(h, hipMalloc((void **)&h->d_jump_slots, (size_t)slots * sizeof(uint32_t)));
    HIP_TRY(h, hipMemsetAsync(h->d_jump_slots, 0, (size_t)slots * sizeof(uint32_t), h->stream));
    h->jump_slot_count = slots;
    h->jump_slot_threads = wg_threads;
    return VRC_OK;
}

int ensure_hits(vrc_caster *h) {
    if (h->d_hits || !h->d_viewport) return VRC_OK;
    const size_t npix = (size_t)h->width * (size_t)std::max(h->buffer_rows, 1);
    HIP_TRY(h, hipMalloc((void **)&h->d_hits, 32 * npix));
    HIP_TRY(h, hipMemsetAsync(h->d_hits, 0, 32 * npix, h->stream));
    return VRC_OK;
}

// Is this host address page-locked (hipHostMalloc / hipHostRegister)?  hipMemcpyAsync into pageable memory blocks the
// calling thread copy by copy, which would serialise the tiles of a multi-GPU read-back.
bool host_byte_is_pinned(const void *p) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    const hipError_t e = hipPointerGetAttributes(&a, p);
    (void)hipGetLastError();
    return e == hipSuccess && a.type == hipMemoryTypeHost;
}
// the whole destination [p, p + bytes) must be page-locked: a buffer pinned only in part (vrc_pin_host_buffer with a
// smaller size, or a sub-range of a larger array) is treated as pageable and staged.  Registered ranges are contiguous,
// and two adjacent registrations are still page-locked memory, so the first and the last byte decide.
bool host_is_pinned(const void *p, size_t bytes) {
    if (!p || !bytes) return false;
    return host_byte_is_pinned(p) && host_byte_is_pinned((const char *)p + bytes - 1);
}

// device rows -> the caller's full-frame buffer, `bpp` bytes per pixel.  stage: copy into this rank's pinned staging
// buffer instead (finish_rows_out moves them on after the stream has been waited for).
int copy_rows_out(vrc_caster *h, const void *dev, size_t bpp, void *host, bool stage) {
    const size_t row = (size_t)h->width * bpp;
    if (stage) {
        const size_t bytes = row * (size_t)std::max(h->buffer_rows, 1);
        if (h->pinned_stage_bytes < bytes) {
            if (h->pinned_stage) (void)hipHostFree(h->pinned_stage);
            h->pinned_stage = nullptr; h->pinned_stage_bytes = 0;
            HIP_TRY(h, hipHostMalloc(&h->pinned_stage, bytes, hipHostMallocDefault));
            h->pinned_stage_bytes = bytes;
        }
        HIP_TRY(h, hipMemcpyAsync(h->pinned_stage, dev, row * (size_t)(h->sliced ? h->buffer_rows : h->height), hipMemcpyDeviceToHost, h->stream));
        return VRC_OK;
    }
    if (!h->sliced) {
        HIP_TRY(h, hipMemcpyAsync(host, dev, row * (size_t)h->height, hipMemcpyDeviceToHost, h->stream));
        return VRC_OK;
    }
    for (const RowRun &r : row_runs(h, true))
        HIP_TRY(h, hipMemcpyAsync((char *)host + row * (size_t)r.y0, (const char *)dev + row * (size_t)r.b0, row * (size_t)r.n,
                                  hipMemcpyDeviceToHost, h->stream));
    return VRC_OK;
}
// second half of a staged read-back (after the rank's stream has been waited for): staging buffer -> the caller's frame
void finish_rows_out(vrc_caster *h, size_t bpp, void *host) {
    const size_t row = (size_t)h->width * bpp;
    if (!h->sliced) { memcpy(host, h->pinned_stage, row * (size_t)h->height); return; }
    for (const RowRun &r : row_runs(h, true))
        memcpy((char *)host + row * (size_t)r.y0, (const char *)h->pinned_stage + row * (size_t)r.b0, row * (size_t)r.n);
}

int sync_one(vrc_caster *h) {
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    drain_events(h);
    if (h->wd_flag && *(volatile unsigned int *)h->wd_flag) {
        *(volatile unsigned int *)h->wd_flag = 0;
        return fail(h, VRC_ERR_DEVICE, "the kernel's round watchdog stopped a wavefront: the frame is invalid (setting watchdog_rounds)");
    }
    return VRC_OK;
}

}  // namespace

extern "C" {

int vrc_device_count(int *count) {
    if (!count) return VRC_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return VRC_ERR_DEVICE; }
    *count = n;
    return VRC_OK;
}

int vrc_create(int device_ordinal, vrc_caster **out) {
    if (!out) return VRC_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return VRC_ERR_DEVICE;   // no GPU: no CPU fallback
    if (device_ordinal < 0 || device_ordinal >= n) return VRC_ERR_INVALID_ARGUMENT;
    vrc_caster *h = new vrc_caster();
    h->device = device_ordinal;
    if (hipSetDevice(device_ordinal) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **)&h->d_counters, sizeof(unsigned long long) * vrc::kCtrCount) != hipSuccess ||
        hipMalloc((void **)&h->d_frame, sizeof(int32_t) * 4) != hipSuccess ||
        hipHostMalloc((void **)&h->wd_flag, sizeof(unsigned int), hipHostMallocMapped) != hipSuccess) {
        delete h;
        return VRC_ERR_DEVICE;
    }
    *h->wd_flag = 0;
    (void)hipMemset(h->d_counters, 0, sizeof(unsigned long long) * vrc::kCtrCount);
    (void)hipMemset(h->d_frame, 0, sizeof(int32_t) * 4);
    *out = h;
    return VRC_OK;
}

int vrc_create_group_ex(const int32_t *device_ordinals, int32_t n, int32_t band_rows, uint32_t flags, vrc_caster **out) {
    if (!out || !device_ordinals || n < 1 || band_rows < vrc::kTileH || band_rows % vrc::kTileH) return VRC_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    vrc_caster *root = nullptr;
    int rc = vrc_create(device_ordinals[0], &root);
    if (rc != VRC_OK) return rc;
    root->tile_rank = 0; root->tile_world = n; root->band_rows = band_rows; root->sliced = n > 1;
    std::string notes;
    for (int32_t r = 1; r < n; r++) {
        vrc_caster *q = nullptr;
        rc = vrc_create(device_ordinals[r], &q);
        if (rc != VRC_OK) { vrc_destroy(root); return rc; }
        q->tile_rank = r; q->tile_world = n; q->band_rows = band_rows; q->sliced = true; q->is_peer = true;
        q->own_copy = (flags & VRC_GROUP_OWN_COPIES) != 0;
        root->peers.push_back(q);
        if (q->device != root->device) {                       // SVO fan-out goes device to device over xGMI
            int can = 0;
            q->peer_access = 0;
            if (hipDeviceCanAccessPeer(&can, q->device, root->device) == hipSuccess && can) {
                (void)hipSetDevice(q->device);
                const hipError_t e = hipDeviceEnablePeerAccess(root->device, 0);
                if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) q->peer_access = 1;
            }
            (void)hipGetLastError();
            if (!q->peer_access) {
                char buf[160];
                snprintf(buf, sizeof(buf), "rank %d: no direct peer access from GPU %d to GPU %d, tree copies are staged by the runtime; ",
                         r, q->device, root->device);
                notes += buf;
            }
        }
    }
    (void)hipSetDevice(root->device);
    root->error = notes;                   // not a failure: vrc_last_error right after creation tells which ranks fell back
    *out = root;
    return VRC_OK;
}

int vrc_create_group(const int32_t *device_ordinals, int32_t n, int32_t band_rows, vrc_caster **out) {
    // VRC_GROUP_OWN_COPIES=1 in the environment: rehearse the distinct-GPU code paths on a box with one GPU
    const char *env = getenv("VRC_GROUP_OWN_COPIES");
    return vrc_create_group_ex(device_ordinals, n, band_rows, (env && env[0] == '1') ? VRC_GROUP_OWN_COPIES : 0u, out);
}

int vrc_group_size(const vrc_caster *h, int32_t *n) {
    if (!h || !n) return VRC_ERR_INVALID_ARGUMENT;
    *n = (int32_t)h->peers.size() + 1;
    return VRC_OK;
}

int vrc_destroy(vrc_caster *h) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    for (vrc_caster *q : h->peers) vrc_destroy(q);
    h->peers.clear();
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    drain_events(h);
    for (auto &p : h->pool) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    release_tree(h);
    release(h->d_map);
    release_viewport_buffers(h); release(h->d_atlas);
    release(h->d_partials); release(h->d_counters); release(h->d_frame);
    release_query_staging(h);
    if (h->wd_flag) (void)hipHostFree(h->wd_flag);
    if (h->pinned_stage) (void)hipHostFree(h->pinned_stage);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return VRC_OK;
}

const char *vrc_last_error(const vrc_caster *h) { return h ? h->error.c_str() : "null handle"; }

int vrc_assign_map(vrc_caster *h, const int8_t *voxels, int32_t dx, int32_t dy, int32_t dz) {
    if (!h || !voxels || dx <= 0 || dy <= 0 || dz <= 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_map: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    release(h->d_map);
    const size_t bytes = (size_t)dx * dy * dz;
    HIP_TRY(h, hipMalloc((void **)&h->d_map, bytes));
    HIP_TRY(h, hipMemcpy(h->d_map, voxels, bytes, hipMemcpyHostToDevice));
    h->map_dim[0] = dx; h->map_dim[1] = dy; h->map_dim[2] = dz;
    h->validated = false;
    FOR_PEERS(h, vrc_assign_map(q, voxels, dx, dy, dz));
    return VRC_OK;
}

int vrc_release_map(vrc_caster *h) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    if (!h->d_map) return fail(h, VRC_ERR_NOT_FOUND, "release_map: no map assigned");
    release(h->d_map);
    release_query_staging(h);
    h->map_dim[0] = h->map_dim[1] = h->map_dim[2] = 0;
    h->validated = false;
    FOR_PEERS(h, vrc_release_map(q));
    return VRC_OK;
}

}  // extern "C"

namespace {

// Give every other rank of the group rank 0's tree: shared when the rank sits on the same GPU, copied device to
// device otherwise (hipMemcpyPeerAsync: xGMI, no host staging; SURVEY 8e "peer fan-out").
int fan_out_tree(vrc_caster *h) {
    const vrc_tree *s = h->tree.get();
    if (!h->peers.empty()) {                                   // the copies run on the peers' streams: rank 0's tree must be complete
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    for (size_t i = 0; i < h->peers.size(); i++) {
        vrc_caster *q = h->peers[i];
        release_tree(q);
        if (q->device == h->device && !q->own_copy) {
            q->tree = h->tree;                                 // one tree, one table, one set of boxes for the ranks of one GPU
            q->owns_desc = false;
        } else {
            HIP_TRY(h, hipSetDevice(q->device));
            std::shared_ptr<vrc_tree> t = new_tree(q->device);
            t->n_desc = s->n_desc;
            HIP_TRY(h, hipMalloc((void **)&t->d_desc, s->n_desc * sizeof(uint64_t)));
            HIP_TRY(h, hipMemcpyPeerAsync(t->d_desc, q->device, s->d_desc, h->device, s->n_desc * sizeof(uint64_t), q->stream));
            if (s->d_attach_lookup && s->d_attach) {
                t->n_attach = s->n_attach;
                HIP_TRY(h, hipMalloc((void **)&t->d_attach_lookup, s->n_desc * sizeof(uint32_t)));
                HIP_TRY(h, hipMalloc((void **)&t->d_attach, std::max<uint64_t>(s->n_attach, 1) * sizeof(uint64_t)));
                HIP_TRY(h, hipMemcpyPeerAsync(t->d_attach_lookup, q->device, s->d_attach_lookup, h->device, s->n_desc * sizeof(uint32_t), q->stream));
                HIP_TRY(h, hipMemcpyPeerAsync(t->d_attach, q->device, s->d_attach, h->device,
                                              std::max<uint64_t>(s->n_attach, 1) * sizeof(uint64_t), q->stream));
            }
            q->tree = std::move(t);
        }
        VRC_TRY(set_setting(q, "octree_root_index", "OCTREE_ROOT_INDEX", setting_or(h, "octree_root_index", 0)));
    }
    for (vrc_caster *q : h->peers)
        if (q->owns_desc) { HIP_TRY(h, hipSetDevice(q->device)); HIP_TRY(h, hipStreamSynchronize(q->stream)); }
    HIP_TRY(h, hipSetDevice(h->device));
    return VRC_OK;
}

// The one way a handle gets a tree (after drop_trees): attach the complete tree, point the root setting at it, give it to the
// peers.  adopted: the tree is another handle's too (vrc_assign_octree_from).
int install_tree(vrc_caster *h, std::shared_ptr<vrc_tree> tree, uint64_t root_index, bool adopted = false) {
    h->tree = std::move(tree);
    h->owns_desc = !adopted;
    VRC_TRY(set_setting(h, "octree_root_index", "OCTREE_ROOT_INDEX", (int64_t)root_index));   // CLCaster.cpp:113
    return fan_out_tree(h);
}

bool lookup_in_range(const uint32_t *lookup, size_t n, uint64_t n_attach) {
    const uint64_t limit = std::max<uint64_t>(n_attach, 1);
    for (size_t i = 0; i < n; i++)
        if (lookup[i] >= limit) return false;
    return true;
}

}  // namespace

extern "C" {

int vrc_assign_octree(vrc_caster *h, const uint64_t *descriptors, uint64_t n, uint64_t root_index) {
    if (!h || !descriptors || n == 0 || root_index >= n) return fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_octree: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    drop_trees(h);
    std::shared_ptr<vrc_tree> t = new_tree(h->device);
    HIP_TRY(h, hipMalloc((void **)&t->d_desc, n * sizeof(uint64_t)));
    HIP_TRY(h, hipMemcpy(t->d_desc, descriptors, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    t->n_desc = n;
    return install_tree(h, std::move(t), root_index);
}

// The tree another handle on the same GPU already holds, adopted instead of uploaded again: one descriptor array, one coarse
// table, one set of empty boxes between the two (vrc_tree).  The arrays live until the last handle lets go of them.
int vrc_assign_octree_from(vrc_caster *h, vrc_caster *src) {
    if (!h || !src || h == src) return fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_octree_from: bad argument");
    if (!src->tree) return fail(h, VRC_ERR_NOT_READY, "assign_octree_from: the source handle has no octree");
    if (src->device != h->device) return fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_octree_from: the handles sit on different GPUs (%d, %d)", h->device, src->device);
    HIP_TRY(h, hipSetDevice(h->device));
    std::shared_ptr<vrc_tree> keep = src->tree;                    // (src may be a peer of h's own group)
    const int64_t root = setting_or(src, "octree_root_index", 0);
    drop_trees(h);
    return install_tree(h, std::move(keep), (uint64_t)root, true);
}

int vrc_assign_octree_attachments(vrc_caster *h, const uint32_t *lookup, uint64_t n_lookup,
                                  const uint64_t *attachments, uint64_t n_attachments) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    if (!h->tree) return fail(h, VRC_ERR_NOT_READY, "assign_octree_attachments: assign the octree first");
    HIP_TRY(h, hipSetDevice(h->device));
    // the arguments are checked before anything is touched: a rejected call leaves every rank as it was
    const bool have = lookup && n_lookup && attachments && n_attachments;
    if (have) {
        if (n_lookup != h->tree->n_desc)
            return fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_octree_attachments: lookup must have one entry per descriptor");
        if (!lookup_in_range(lookup, (size_t)n_lookup, n_attachments))
            return fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_octree_attachments: a lookup entry points past the attachment buffer");
    }
    // from here on every rank drops its old buffers first, so that a device failure half-way can never leave two ranks
    // of one frame with different materials (ranks that share rank 0's arrays just forget the pointers)
    // (the buffers belong to the TREE: every handle that shares it renders with the new materials from its next frame on)
    auto drop = [](vrc_caster *q) {
        vrc_tree *t = q->tree.get();
        if (t) {
            std::lock_guard<std::mutex> lock(t->guard);            // (another holder's frame reads these pointers under the guard)
            (void)hipSetDevice(t->device); release(t->d_attach_lookup); release(t->d_attach); t->n_attach = 0;
            t->cap_lookup = t->cap_attach = 0;
        }
        q->validated = false;
    };
    for (vrc_caster *q : h->peers) drop(q);
    drop(h);
    HIP_TRY(h, hipSetDevice(h->device));
    vrc_tree *t = h->tree.get();
    if (have) {
        std::lock_guard<std::mutex> lock(t->guard);
        HIP_TRY(h, hipMalloc((void **)&t->d_attach_lookup, n_lookup * sizeof(uint32_t)));
        HIP_TRY(h, hipMemcpy(t->d_attach_lookup, lookup, n_lookup * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMalloc((void **)&t->d_attach, n_attachments * sizeof(uint64_t)));
        HIP_TRY(h, hipMemcpy(t->d_attach, attachments, n_attachments * sizeof(uint64_t), hipMemcpyHostToDevice));
        t->n_attach = n_attachments;
    }
    if (h->peers.empty()) return VRC_OK;
    // ranks with their own copy of the descriptors: only the attachment buffers change
    for (vrc_caster *q : h->peers) {
        vrc_tree *tq = q->tree.get();
        if (tq && tq != t && t->d_attach_lookup && t->d_attach) {   // (no tree: the rank's copy failed in the fan-out)
            HIP_TRY(h, hipSetDevice(q->device));
            HIP_TRY(h, hipMalloc((void **)&tq->d_attach_lookup, t->n_desc * sizeof(uint32_t)));
            HIP_TRY(h, hipMalloc((void **)&tq->d_attach, t->n_attach * sizeof(uint64_t)));
            HIP_TRY(h, hipMemcpyPeer(tq->d_attach_lookup, q->device, t->d_attach_lookup, h->device, t->n_desc * sizeof(uint32_t)));
            HIP_TRY(h, hipMemcpyPeer(tq->d_attach, q->device, t->d_attach, h->device, t->n_attach * sizeof(uint64_t)));
            tq->n_attach = t->n_attach;
        }
    }
    HIP_TRY(h, hipSetDevice(h->device));
    return VRC_OK;
}

}  // extern "C"

namespace {
// file -> device through two pinned staging buffers: the read of chunk k+1 overlaps the copy of chunk k.
// check (optional) looks at every staged chunk before it is sent.
int stream_to_device(vrc_caster *h, FILE *f, void *dst, size_t bytes, void *stage[2], size_t chunk,
                     bool (*check)(const void *, size_t, uint64_t), uint64_t check_arg) {
    hipEvent_t done[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; i++) HIP_TRY(h, hipEventCreateWithFlags(&done[i], hipEventDisableTiming));
    int rc = VRC_OK;
    size_t off = 0;
    for (int k = 0; off < bytes; k ^= 1) {
        const size_t n = std::min(chunk, bytes - off);
        if (hipEventSynchronize(done[k]) != hipSuccess) { rc = fail(h, VRC_ERR_DEVICE, "assign_octree_file: event wait failed"); break; }
        if (fread(stage[k], 1, n, f) != n) { rc = fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_octree_file: file is truncated"); break; }
        if (check && !check(stage[k], n, check_arg)) { rc = fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_octree_file: a lookup entry points past the attachment buffer"); break; }
        if (hipMemcpyAsync((char *)dst + off, stage[k], n, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipEventRecord(done[k], h->stream) != hipSuccess) { rc = fail(h, VRC_ERR_DEVICE, "assign_octree_file: upload failed"); break; }
        off += n;
    }
    (void)hipStreamSynchronize(h->stream);
    for (int i = 0; i < 2; i++) (void)hipEventDestroy(done[i]);
    return rc;
}
bool check_lookup_chunk(const void *p, size_t bytes, uint64_t n_attach) {
    return lookup_in_range((const uint32_t *)p, bytes / sizeof(uint32_t), n_attach);
}
}  // namespace

extern "C" {

int vrc_assign_octree_file(vrc_caster *h, const char *path, uint32_t *dim) {
    if (!h || !path || !dim) return fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_octree_file: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    FILE *f = fopen(path, "rb");
    if (!f) return fail(h, VRC_ERR_NOT_FOUND, "assign_octree_file: cannot open '%s'", path);
    char magic[8];
    uint32_t flags = 0;
    uint64_t root = 0, n = 0, na = 0;
    const bool header = fread(magic, 1, 8, f) == 8 && memcmp(magic, "VRCSVO01", 8) == 0 && fread(dim, 4, 1, f) == 1 &&
                        fread(&flags, 4, 1, f) == 1 && fread(&root, 8, 1, f) == 1 && fread(&n, 8, 1, f) == 1 &&
                        fread(&na, 8, 1, f) == 1 && n > 0 && root < n && *dim >= 2 && (*dim & (*dim - 1)) == 0;
    if (!header) { fclose(f); return fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_octree_file: '%s' is not a VRCSVO01 file", path); }
    drop_trees(h);
    const size_t chunk = (size_t)setting_or(h, "upload_chunk_bytes", 64 << 20);
    void *stage[2] = {nullptr, nullptr};
    int rc = VRC_OK;
    if (chunk < 4096 || hipHostMalloc(&stage[0], chunk, hipHostMallocDefault) != hipSuccess || hipHostMalloc(&stage[1], chunk, hipHostMallocDefault) != hipSuccess)
        rc = fail(h, VRC_ERR_OUT_OF_MEMORY, "assign_octree_file: no pinned staging memory");
    std::shared_ptr<vrc_tree> t = new_tree(h->device);
    if (rc == VRC_OK && hipMalloc((void **)&t->d_desc, n * sizeof(uint64_t)) != hipSuccess)
        rc = fail(h, VRC_ERR_OUT_OF_MEMORY, "assign_octree_file: %llu descriptors do not fit in device memory", (unsigned long long)n);
    if (rc == VRC_OK) rc = stream_to_device(h, f, t->d_desc, n * sizeof(uint64_t), stage, chunk, nullptr, 0);
    if (rc == VRC_OK && (flags & 1u)) {
        if (hipMalloc((void **)&t->d_attach_lookup, n * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc((void **)&t->d_attach, (na ? na : 1) * sizeof(uint64_t)) != hipSuccess)
            rc = fail(h, VRC_ERR_OUT_OF_MEMORY, "assign_octree_file: attachment buffers do not fit in device memory");
        if (rc == VRC_OK && na == 0 && hipMemset(t->d_attach, 0x05, sizeof(uint64_t)) != hipSuccess)
            rc = fail(h, VRC_ERR_DEVICE, "assign_octree_file: memset failed");
        if (rc == VRC_OK) rc = stream_to_device(h, f, t->d_attach_lookup, n * sizeof(uint32_t), stage, chunk, check_lookup_chunk, na);
        if (rc == VRC_OK) rc = stream_to_device(h, f, t->d_attach, na * sizeof(uint64_t), stage, chunk, nullptr, 0);
    }
    fclose(f);
    for (int i = 0; i < 2; i++) if (stage[i]) (void)hipHostFree(stage[i]);
    if (rc != VRC_OK) return rc;                                   // (the half-filled tree goes with t)
    t->n_desc = n; t->n_attach = (flags & 1u) ? std::max<uint64_t>(na, 1) : 0;
    return install_tree(h, std::move(t), root);
}

int vrc_build_shell_terrain(vrc_caster *h, uint32_t depth, uint64_t seed, int32_t thickness, int32_t octave_floor,
                            uint32_t flags, uint64_t validate_samples, const int32_t *probe_xy, uint32_t n_probe,
                            int32_t *probe_lohi, vrc_build_info *info) {
    if (!h || depth < 3 || depth > 16 || thickness < 0 || octave_floor < 0)
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "build_shell_terrain: need 3 <= depth <= 16, thickness >= 0, octave_floor >= 0");
    HIP_TRY(h, hipSetDevice(h->device));
    const bool count_only = (flags & VRC_BUILD_COUNT_ONLY) != 0;
    if (!count_only) drop_trees(h);
    uint64_t *d = nullptr;
    vrc_build_info bi;
    std::string err;
    const int rc = vrc::build_shell_terrain_device(h->stream, depth, seed, thickness, octave_floor, flags, validate_samples, probe_xy,
                                                   n_probe, probe_lohi, &d, &bi, err);
    if (info) *info = bi;
    if (rc != VRC_OK) return fail(h, rc, "build_shell_terrain: %s", err.c_str());
    if (count_only) return VRC_OK;
    return install_tree(h, new_tree(h->device, d, bi.n_descriptors), bi.root_index);
}

int vrc_build_heightfield(vrc_caster *h, uint32_t depth, const uint16_t *hi, const uint16_t *lo, uint32_t flags,
                          uint64_t validate_samples, vrc_build_info *info) {
    if (!h || depth < 3 || depth > 16 || !hi)
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "build_heightfield: need 3 <= depth <= 16 and a height field");
    const size_t n = (size_t)1 << (2 * depth);
    for (size_t i = 0; i < n; i++)
        if (hi[i] >= (1u << depth) || (lo && lo[i] > hi[i]))
            return fail(h, VRC_ERR_INVALID_ARGUMENT, "build_heightfield: column %zu needs lo <= hi < dim", i);
    HIP_TRY(h, hipSetDevice(h->device));
    const bool count_only = (flags & VRC_BUILD_COUNT_ONLY) != 0;
    if (!count_only) drop_trees(h);
    uint64_t *d = nullptr;
    vrc_build_info bi;
    std::string err;
    const int rc = vrc::build_columns_device(h->stream, depth, 0, 0, 0, hi, lo, flags, validate_samples, nullptr, 0, nullptr, &d, &bi, err);
    if (info) *info = bi;
    if (rc != VRC_OK) return fail(h, rc, "build_heightfield: %s", err.c_str());
    if (count_only) return VRC_OK;
    return install_tree(h, new_tree(h->device, d, bi.n_descriptors), bi.root_index);
}

int vrc_build_dense_grid(vrc_caster *h, uint32_t depth, const int8_t *grid, uint32_t flags, uint64_t validate_samples,
                         vrc_build_info *info) {
    if (!h || depth < 3 || depth > 12)
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "build_dense_grid: need 3 <= depth <= 12");
    const int32_t dim = (int32_t)1 << depth;
    if (!grid && !(h->d_map && h->map_dim[0] == dim && h->map_dim[1] == dim && h->map_dim[2] == dim))
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "build_dense_grid: no grid given and no %d^3 map assigned (vrc_assign_map) to build from", dim);
    HIP_TRY(h, hipSetDevice(h->device));
    const bool count_only = (flags & VRC_BUILD_COUNT_ONLY) != 0;
    if (!count_only) drop_trees(h);
    uint64_t *d = nullptr;
    vrc_build_info bi;
    std::string err;
    uint32_t *lookup = nullptr;
    uint64_t *attach = nullptr, n_attach = 0;
    const int rc = vrc::build_grid_device(h->stream, depth, grid, grid ? nullptr : h->d_map, flags, validate_samples, &d, &lookup, &attach,
                                          &n_attach, &bi, err);
    if (info) *info = bi;
    if (rc != VRC_OK) return fail(h, rc, "build_dense_grid: %s", err.c_str());
    if (count_only) return VRC_OK;
    std::shared_ptr<vrc_tree> t = new_tree(h->device, d, bi.n_descriptors);
    t->d_attach_lookup = lookup; t->d_attach = attach; t->n_attach = n_attach;
    return install_tree(h, std::move(t), bi.root_index);
}

int vrc_read_descriptors(vrc_caster *h, uint64_t first, uint64_t count, uint64_t *out) {
    if (!h || !out) return VRC_ERR_INVALID_ARGUMENT;
    if (!h->tree) return fail(h, VRC_ERR_NOT_READY, "read_descriptors: no octree assigned");
    if (first > h->tree->n_desc || count > h->tree->n_desc - first) return fail(h, VRC_ERR_INVALID_ARGUMENT, "read_descriptors: range past the array");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpy(out, h->tree->d_desc + first, count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VRC_OK;
}

// the materials of the resident octree, as vrc_assign_octree_attachments takes them (tests, tools: an edited tree's are made on the device)
int vrc_read_attachments(vrc_caster *h, uint32_t *lookup, uint64_t *attachments, uint64_t capacity, uint64_t *n_attachments) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    vrc_tree *t = h->tree.get();
    if (!t) return fail(h, VRC_ERR_NOT_READY, "read_attachments: no octree assigned");
    std::lock_guard<std::mutex> lock(t->guard);
    const bool have = t->d_attach_lookup && t->d_attach;
    const uint64_t n = have ? std::max<uint64_t>(t->n_attach, 1) : 0;
    if (n_attachments) *n_attachments = n;
    if (!have || (!lookup && !attachments)) return VRC_OK;
    if (attachments && capacity < n) return fail(h, VRC_ERR_INVALID_ARGUMENT, "read_attachments: %llu slots, room for %llu", (unsigned long long)n, (unsigned long long)capacity);
    DeviceRestore restore;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (lookup) HIP_TRY(h, hipMemcpy(lookup, t->d_attach_lookup, t->n_desc * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (attachments) HIP_TRY(h, hipMemcpy(attachments, t->d_attach, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VRC_OK;
}

int vrc_octree_size(vrc_caster *h, uint64_t *n_descriptors, uint64_t *root_index) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    if (!h->tree) return fail(h, VRC_ERR_NOT_READY, "octree_size: no octree assigned");
    if (n_descriptors) *n_descriptors = h->tree->n_desc;
    if (root_index) *root_index = (uint64_t)setting_or(h, "octree_root_index", 0);
    return VRC_OK;
}

int vrc_release_octree(vrc_caster *h) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    if (!h->tree) return fail(h, VRC_ERR_NOT_FOUND, "release_octree: no octree assigned");
    drop_trees(h);
    release_query_staging(h);
    return VRC_OK;
}

int vrc_create_viewport(vrc_caster *h, int32_t width, int32_t height, float v_fov, float h_fov) {
    (void)v_fov; (void)h_fov;              // ignored by the reference too (CLCaster.cpp:233-275)
    if (!h || width <= 0 || height <= 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "create_viewport: bad size");
    VRC_TRY(install_viewport(h, width, height, nullptr));
    FOR_PEERS(h, vrc_create_viewport(q, width, height, v_fov, h_fov));
    return VRC_OK;
}

int vrc_create_viewport_table(vrc_caster *h, int32_t width, int32_t height, const float *table) {
    if (!h || !table || width <= 0 || height <= 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "create_viewport_table: bad argument");
    VRC_TRY(install_viewport(h, width, height, table));
    FOR_PEERS(h, vrc_create_viewport_table(q, width, height, table));
    return VRC_OK;
}

int vrc_release_viewport(vrc_caster *h) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    if (!h->d_viewport) return fail(h, VRC_ERR_NOT_FOUND, "release_viewport: no viewport");
    release_viewport_buffers(h);
    release_query_staging(h);
    h->width = h->height = h->buffer_rows = 0; h->validated = false;
    FOR_PEERS(h, vrc_release_viewport(q));
    return VRC_OK;
}

int vrc_create_texture_atlas(vrc_caster *h, const uint8_t *rgba8, int32_t width, int32_t height,
                             int32_t tile_w, int32_t tile_h) {
    if (!h || !rgba8 || width <= 0 || height <= 0 || tile_w <= 0 || tile_h <= 0)
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "create_texture_atlas: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    release(h->d_atlas);
    HIP_TRY(h, hipMalloc((void **)&h->d_atlas, (size_t)4 * width * height));
    HIP_TRY(h, hipMemcpy(h->d_atlas, rgba8, (size_t)4 * width * height, hipMemcpyHostToDevice));
    h->atlas_w = width; h->atlas_h = height; h->tile_w = tile_w; h->tile_h = tile_h;
    h->validated = false;
    FOR_PEERS(h, vrc_create_texture_atlas(q, rgba8, width, height, tile_w, tile_h));
    return VRC_OK;
}

int vrc_assign_camera(vrc_caster *h, const float *direction2, const float *position3) {
    if (!h || !direction2 || !position3) return fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_camera: null pointer");
    h->cam_dir = direction2; h->cam_pos = position3;
    h->validated = false;
    FOR_PEERS(h, vrc_assign_camera(q, direction2, position3));
    return VRC_OK;
}

int vrc_assign_camera_trig(vrc_caster *h, const float *trig4) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    h->cam_trig = trig4;                   // (NULL: back to sinf / cosf of the live direction)
    FOR_PEERS(h, vrc_assign_camera_trig(q, trig4));
    return VRC_OK;
}

int vrc_release_camera(vrc_caster *h) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    h->cam_dir = h->cam_pos = nullptr; h->cam_trig = nullptr; h->validated = false;
    FOR_PEERS(h, vrc_release_camera(q));
    return VRC_OK;
}

int vrc_assign_lights(vrc_caster *h, const float *packed, const int32_t *light_count) {
    if (!h || !packed || !light_count) return fail(h, VRC_ERR_INVALID_ARGUMENT, "assign_lights: null pointer");
    h->lights = packed; h->light_count = light_count;
    h->validated = false;
    FOR_PEERS(h, vrc_assign_lights(q, packed, light_count));
    return VRC_OK;
}

int vrc_setting_add(vrc_caster *h, const char *name, const char *define, int64_t value) {
    if (!h || !name) return VRC_ERR_INVALID_ARGUMENT;
    VRC_TRY(set_setting(h, name, define, value));
    FOR_PEERS(h, vrc_setting_add(q, name, define, value));
    return VRC_OK;
}

int vrc_setting_set(vrc_caster *h, const char *name, int64_t value) {
    if (!h || !name) return VRC_ERR_INVALID_ARGUMENT;
    int i = find_setting(h, name);
    if (i < 0) return fail(h, VRC_ERR_NOT_FOUND, "overwrite_setting: no setting named '%s'", name);   // CLCaster.cpp:1096-1100
    retry_derived(h, name);
    h->settings[i].value = value;
    FOR_PEERS(h, vrc_setting_set(q, name, value));
    return VRC_OK;
}

int vrc_setting_get(vrc_caster *h, const char *name, int64_t *value) {
    if (!h || !name || !value) return VRC_ERR_INVALID_ARGUMENT;
    int i = find_setting(h, name);
    if (i < 0) return fail(h, VRC_ERR_NOT_FOUND, "no setting named '%s'", name);
    *value = h->settings[i].value;
    return VRC_OK;
}

int vrc_set_row_tiling(vrc_caster *h, int32_t rank, int32_t world, int32_t band_rows) {
    if (!h || world < 1 || rank < 0 || rank >= world || band_rows < vrc::kTileH || band_rows % vrc::kTileH)
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "set_row_tiling: need 0 <= rank < world and band_rows a multiple of 8");
    if (!h->peers.empty() || h->is_peer) return fail(h, VRC_ERR_INVALID_ARGUMENT, "set_row_tiling: the ranks of a group are tiled by vrc_create_group");
    if (h->sliced) return fail(h, VRC_ERR_INVALID_ARGUMENT, "set_row_tiling: this handle holds a row slice (vrc_set_row_slice); release the viewport first");
    h->tile_rank = rank; h->tile_world = world; h->band_rows = band_rows;
    return VRC_OK;
}

int vrc_set_row_slice(vrc_caster *h, int32_t rank, int32_t world, int32_t band_rows) {
    if (!h || world < 1 || rank < 0 || rank >= world || band_rows < vrc::kTileH || band_rows % vrc::kTileH)
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "set_row_slice: need 0 <= rank < world and band_rows a multiple of 8");
    if (!h->peers.empty() || h->is_peer) return fail(h, VRC_ERR_INVALID_ARGUMENT, "set_row_slice: the ranks of a group are sliced by vrc_create_group");
    if (h->d_viewport) return fail(h, VRC_ERR_NOT_READY, "set_row_slice: call it before create_viewport (the buffers are sized by it)");
    h->tile_rank = rank; h->tile_world = world; h->band_rows = band_rows; h->sliced = world > 1;
    return VRC_OK;
}

int vrc_validate(vrc_caster *h) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    h->validated = false;
    // CLCaster.cpp:165-184: camera, map, viewport image + matrix must be set
    if (!h->cam_dir || !h->cam_pos) return fail(h, VRC_ERR_NOT_READY, "validate: camera not assigned");
    if (!h->d_viewport || !h->d_image) return fail(h, VRC_ERR_NOT_READY, "validate: viewport not created");
    if (!h->lights) return fail(h, VRC_ERR_NOT_READY, "validate: lights not assigned");
    if (!h->d_atlas) return fail(h, VRC_ERR_NOT_READY, "validate: texture atlas not created");
    if (!h->tree) return fail(h, VRC_ERR_NOT_READY, "validate: octree not assigned");
    if (find_setting(h, "octree_dimensions") < 0) return fail(h, VRC_ERR_NOT_READY, "validate: setting octree_dimensions missing");
    if (find_setting(h, "using_octree") < 0) return fail(h, VRC_ERR_NOT_READY, "validate: setting using_octree missing");
    const int64_t dim = setting_or(h, "octree_dimensions", 0);
    const int n = log2_exact(dim);
    if (n < 1) return fail(h, VRC_ERR_INVALID_ARGUMENT, "validate: octree_dimensions must be a power of two >= 2");
    if (n > vrc::kMaxLevels) return fail(h, VRC_ERR_LIMIT, "validate: octree deeper than %d levels", vrc::kMaxLevels);
    const int64_t root = setting_or(h, "octree_root_index", 0);
    if (root < 0 || (uint64_t)root >= h->tree->n_desc) return fail(h, VRC_ERR_INVALID_ARGUMENT, "validate: octree_root_index out of range");
    if (setting_or(h, "using_octree", 0) != 0) {
        if (!h->d_map) return fail(h, VRC_ERR_NOT_READY, "validate: dense map not assigned (using_octree != 0 selects the array branch)");
    }
    if (h->atlas_w / h->tile_w <= 0 || h->atlas_h / h->tile_h <= 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "validate: tile larger than atlas");
    h->validated = true;
    // the reference pays its one-off cost here (the kernel build, CLCaster.cpp:157-206); so do we: the structures the SVO kernels
    // derive from the tree are built now, not inside the first frame.  (each rank of a group prepares in its own vrc_validate)
    if (setting_or(h, "using_octree", 0) == 0) {
        const int rc = prepare_one(h);
        if (rc != VRC_OK) { h->validated = false; return rc; }
    }
    FOR_PEERS(h, vrc_validate(q));
    return VRC_OK;
}

int vrc_prepare(vrc_caster *h) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    VRC_TRY(prepare_one(h));
    FOR_PEERS(h, prepare_one(q));
    if (!h->peers.empty()) HIP_TRY(h, hipSetDevice(h->device));
    return VRC_OK;
}

}  // extern "C"

namespace {

// Build-or-remember-failure of one derived structure.  `have`: it exists; it is kept when it was built for `want`.  Else drop()
// frees it and build() makes it anew -- unless just this (`want_failed`) failed before and the host has not asked again
// (retry_derived).  A failure leaves no structure behind, only its key and the reason: what is missing, then the runtime's error text.
std::string missing(const TableKey &k) { return "no coarse table (level " + std::to_string(k.log2) + ")"; }
std::string missing(const BoxKey &) { return "no empty boxes"; }
template <class Key, class Drop, class Build>
void rebuild(Derived<Key> &d, bool have, const Key &want, const Key &want_failed, Drop drop, Build build) {
    if (have && d.built == want) return;
    drop();
    d.built = Key{};
    if (d.gave_up && d.failed == want_failed) return;
    const hipError_t e = build();
    if (e != hipSuccess) {
        (void)hipGetLastError();
        drop();
        d.gave_up = true; d.failed = want_failed;
        d.note = missing(want_failed) + ": " + hipGetErrorString(e) + "; ";
    } else {
        d.built = want;
        d.gave_up = false; d.note.clear();
    }
}

// The structures the SVO kernels derive from a tree, for these settings: built when missing or built for another (root, depth,
// level); the kernel parameters get the pointers.  The caller holds t->guard.  Both structures are optional accelerations: when
// their memory cannot be had the frame is rendered without them (the table-less / box-less kernel instances); the reason is kept
// with the tree and reported by vrc_memory_usage2, and the build is tried again when what is asked for changes.
void derive_from_tree(vrc_caster *h, vrc_tree *t, int log2_dim, uint64_t root_index, int stepping_mode, vrc::RaycastParams &p) {
    // the levels above coarse_log2 as a dense table (setting coarse_log2: -1 = by depth and tree size, 0 = none), read by both
    // SVO kernels.  By default the finest level of the depth rule whose table is at most 16 x the descriptor array: a sparse
    // tree in a large map does not get a table hundreds of times its own size
    int64_t lc = setting_or(h, "coarse_log2", -1);
    if (lc < 0) {
        lc = vrc::coarse_level_for_depth(log2_dim);
        while (lc >= 1 && ((uint64_t)sizeof(uint64_t) << (3 * lc)) > 16 * sizeof(uint64_t) * t->n_desc && ((uint64_t)sizeof(uint64_t) << (3 * lc)) > (1u << 20)) lc--;
    }
    lc = std::min<int64_t>(lc, std::min(log2_dim - 2, 10));
    const TableKey at{(int)lc, root_index, log2_dim};
    if (lc >= 1 && t->n_desc < (1ULL << 43)) {
        rebuild(t->coarse, t->d_coarse != nullptr, at, at,
                [&] { release(t->d_coarse); release_boxes(t); },   // (the boxes' parallel word belongs to the table's cells)
                [&] {
                    hipError_t e = hipMalloc((void **)&t->d_coarse, sizeof(uint64_t) << (3 * lc));
#ifdef VRC_INDEX_AUDIT
                    if (e == hipSuccess) { AuditExtents x; audit_tree(x, t); x.set(vrc::audit::kCoarse, 1ULL << (3 * lc)); e = audit_publish(x); }
#endif
                    if (e == hipSuccess) e = vrc::launch_coarse_build(t->d_desc, root_index, log2_dim, (int)lc, t->d_coarse, h->stream);
                    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);          // other handles read it from their own streams
                    return e;
                });
        if (t->d_coarse) { p.coarse = t->d_coarse; p.coarse_log2 = (int32_t)lc; }
    } else if (t->d_coarse) {
        release(t->d_coarse); t->coarse.built = TableKey{};   // the setting went to "none": the table goes too
        release_boxes(t);
    }
    // the empty boxes (empty_boxes.hip; setting empty_boxes: -1 = when the tree is small enough for them, 0 = never, 1 = always):
    // 32 bytes per descriptor + 4 per table cell, built like the table they hang on; exact mode only.
    // (Words for the table's cells ALONE -- boxes in the coarse space, octree nodes below it -- would fit any tree; measured:
    // depth 12 1.71 ms against 1.50 with all words and 1.91 without, depth 14 -2 %, depth 16 +4 %: not offered.)
    // Two forms (setting empty_boxes: -1 = by the tree's size, 0 = never, 1 = a word per descriptor and child, 2 = the upper levels only):
    //   * a word per (descriptor, child): trees of up to 2^29 descriptors (16 GB of words) by default.  Beyond that the words are
    //     not only expensive -- gathered from an array of tens of GB they miss the TLB as well as the caches (the depth-15 bench
    //     terrain, 1.4 G descriptors: 4.8 ms with its 45 GB of words, 3.75 without);
    //   * the upper levels only (round 6): box records for the descriptors of the levels the record budget reaches (setting
    //     empty_box_records, default 400 M records = 14 GB of words, at most a quarter of the free device memory; setting
    //     empty_box_levels caps the levels), numbered breadth-first, the nodes below them widened over their empty siblings -- any
    //     tree, also beyond the 2^31 descriptors a 32-bit descriptor index reaches.
    const int64_t want_boxes = setting_or(h, "empty_boxes", -1);
    const bool box_ok = p.coarse != nullptr && stepping_mode == 0 && log2_dim <= 19;
    int box_mode = 0;                                              // 0 none, 1 per descriptor, 2 upper levels
    if (box_ok && want_boxes == 1 && t->n_desc < (1ULL << 31)) box_mode = 1;
    else if (box_ok && want_boxes >= 2) box_mode = 2;
    else if (box_ok && want_boxes < 0) box_mode = t->n_desc <= (1ULL << 29) ? 1 : 2;
    if (box_mode) {
        const int64_t want_levels = box_mode == 2 ? std::max<int64_t>(0, setting_or(h, "empty_box_levels", 0)) : 0;
        const int64_t want_records = box_mode == 2 ? std::max<int64_t>(0, setting_or(h, "empty_box_records", 0)) : 0;
        // (a failure is remembered for the level, root, depth and form alone -- not for the levels and records asked)
        rebuild(t->boxes, t->d_boxes != nullptr, BoxKey{at, box_mode, want_levels, want_records}, BoxKey{at, box_mode},
                [&] { release_boxes(t); },
                [&] {
                    uint64_t *pos_tmp = nullptr;
                    hipEvent_t e0 = nullptr, e1 = nullptr;
                    float ms = 0.f;
                    size_t free_b = 0, total_b = 0;
                    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
                    hipError_t e = hipMalloc((void **)&t->d_box_aux, sizeof(uint32_t) << (3 * lc));
#ifdef VRC_INDEX_AUDIT
                    if (e == hipSuccess) {   // the tree, the table's parallel word and the per-descriptor form's words and positions, as allocated just below
                        AuditExtents x;
                        audit_tree(x, t);
                        x.set(vrc::audit::kBoxAux, 1ULL << (3 * lc));
                        if (box_mode == 1) { x.set(vrc::audit::kBoxes, 8 * t->n_desc); x.set(vrc::audit::kBoxPos, t->n_desc); x.set(vrc::audit::kBoxChild, 0); x.set(vrc::audit::kBoxDesc, 0); }
                        e = audit_publish(x);                  // (the upper-levels form allocates its records itself and publishes them: empty_boxes.hip)
                    }
#endif
                    if (e == hipSuccess) e = hipEventCreate(&e0);
                    if (e == hipSuccess) e = hipEventCreate(&e1);
                    if (e == hipSuccess) e = hipEventRecord(e0, h->stream);
                    if (box_mode == 1) {
                        // (an optional structure must not be what makes the next allocation fail: at most half of what is free right now)
                        if (e == hipSuccess && want_boxes < 0 && t->n_desc > (1ULL << 28) && 40ULL * t->n_desc > free_b / 2) e = hipErrorOutOfMemory;
                        if (e == hipSuccess) e = hipMalloc((void **)&t->d_boxes, sizeof(uint32_t) * 8 * t->n_desc);
                        if (e == hipSuccess) e = hipMalloc((void **)&pos_tmp, sizeof(uint64_t) * t->n_desc);
                        if (e == hipSuccess) e = vrc::launch_box_build(t->d_desc, t->n_desc, root_index, log2_dim, (int)lc, pos_tmp, t->d_boxes, t->d_box_aux, h->stream);
                        if (e == hipSuccess) { t->box_records = t->n_desc; t->box_levels = log2_dim; }
                    } else {
                        uint64_t budget = (uint64_t)want_records;
                        // (measured on the depth-16 terrain, 5.7 G descriptors: 200 M records 4.59 ms, 400 M 4.47, 1.5 G 5.04 -- beyond ~15 GB the
                        // words themselves become TLB misses; without boxes 4.73)
                        if (!budget) budget = std::min<uint64_t>(400000000ULL, (uint64_t)(free_b / 4) / 52);
                        budget = std::min<uint64_t>(budget, 0xffffff00ULL);
                        vrc::BoxUpper u;
                        if (e == hipSuccess) e = vrc::launch_box_build_upper(t->d_desc, root_index, log2_dim, (int)lc, std::max<uint64_t>(budget, 9), (int)want_levels, &u, t->d_box_aux, h->stream);
                        if (e == hipSuccess) {
                            t->d_boxes = u.boxes; t->d_box_child = u.child; t->d_box_desc = u.desc; t->d_box_pos = u.pos;
                            t->box_records = u.count; t->box_levels = u.levels;
                        }
                    }
                    if (e == hipSuccess) e = hipEventRecord(e1, h->stream);
                    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
                    if (e == hipSuccess) (void)hipEventElapsedTime(&ms, e0, e1);
                    if (e == hipSuccess && vrc::box_queries_cut(&t->box_queries_cut) != hipSuccess) { (void)hipGetLastError(); t->box_queries_cut = 0; }
                    if (e0) (void)hipEventDestroy(e0);
                    if (e1) (void)hipEventDestroy(e1);
                    if (pos_tmp) (void)hipFree(pos_tmp);
                    if (e == hipSuccess) t->box_build_seconds = ms * 1e-3;
                    return e;
                });
        if (t->d_boxes) { p.boxes = t->d_boxes; p.box_aux = t->d_box_aux; p.box_child = t->d_box_child; p.box_levels = t->box_levels; }
    }
    // (a handle that switches the boxes off keeps them: they belong to the tree, go with it, and a host that toggles the setting
    // between frames -- tests/soak_jumps_gpu.py does -- must not pay the build again and again)
}

// vrc_prepare for one rank: the derived structures for the settings as they stand
int prepare_one(vrc_caster *h) {
    if (!h->tree) return fail(h, VRC_ERR_NOT_READY, "prepare: octree not assigned");
    const int n = log2_exact(setting_or(h, "octree_dimensions", 0));
    if (n < 1 || n > vrc::kMaxLevels) return fail(h, VRC_ERR_NOT_READY, "prepare: setting octree_dimensions missing or not a power of two in [2, 2^%d]", vrc::kMaxLevels);
    const int64_t root = setting_or(h, "octree_root_index", 0);
    if (root < 0 || (uint64_t)root >= h->tree->n_desc) return fail(h, VRC_ERR_INVALID_ARGUMENT, "prepare: octree_root_index out of range");
    if (setting_or(h, "using_octree", 0) != 0) return VRC_OK;      // the array branch derives nothing
    HIP_TRY(h, hipSetDevice(h->device));
    vrc::RaycastParams p;
    memset(&p, 0, sizeof(p));
    std::lock_guard<std::mutex> lock(h->tree->guard);
    derive_from_tree(h, h->tree.get(), n, (uint64_t)root, (int)setting_or(h, "stepping_mode", 0), p);
    return VRC_OK;
}

int compute_async_one(vrc_caster *h) {
    if (!h->validated) return fail(h, VRC_ERR_NOT_READY, "compute: validate() has not succeeded");
    HIP_TRY(h, hipSetDevice(h->device));
    // The tree's guard is held from here until the kernel is ENQUEUED: another holder of the tree (another host thread, other
    // settings, new materials) that replaces one of its arrays frees the old one with hipFree, which waits for the kernels already
    // enqueued -- never for a frame that has copied the pointers and not launched yet (advisor finding, round 5).
    // (read from the tree itself, under the guard: a handle that shares it may have given it new materials since the last frame)
    vrc_tree *t = h->tree.get();
    std::unique_lock<std::mutex> tree_lock;
    if (t) tree_lock = std::unique_lock<std::mutex>(t->guard);

    // settings stay live after validate() (CLCaster::overwrite_setting needs no recompile, CLCaster.cpp:1087-1109), so
    // the structural ones are checked again here: a bad value is an error return, never a device fault
    vrc::RaycastParams p;
    memset(&p, 0, sizeof(p));
    const bool svo = setting_or(h, "using_octree", 0) == 0;
    const int64_t dim = setting_or(h, "octree_dimensions", 0);
    p.svo = svo ? 1 : 0;
    p.log2_dim = log2_exact(dim);
    if (p.log2_dim < 1 || p.log2_dim > vrc::kMaxLevels)
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "compute: octree_dimensions must be a power of two in [2, 2^%d]", vrc::kMaxLevels);
    const int64_t root = setting_or(h, "octree_root_index", 0);
    if (!t || root < 0 || (uint64_t)root >= t->n_desc) return fail(h, VRC_ERR_INVALID_ARGUMENT, "compute: octree_root_index out of range");
    if (!svo && !h->d_map) return fail(h, VRC_ERR_NOT_READY, "compute: dense map not assigned (using_octree != 0 selects the array branch)");
    if (!h->d_viewport || !h->d_image || !h->d_atlas) return fail(h, VRC_ERR_NOT_READY, "compute: viewport or atlas released since validate()");
    p.stepping_mode = (int32_t)setting_or(h, "stepping_mode", 0);
    if (p.stepping_mode < 0 || p.stepping_mode > 1 || (p.stepping_mode == 1 && !svo))
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "compute: stepping_mode must be 0 (exact) or 1 (node-exit jumps, SVO branch only)");
    p.map = h->d_map;
    if (svo) { p.map_dim[0] = p.map_dim[1] = p.map_dim[2] = (int32_t)dim; }
    else { p.map_dim[0] = h->map_dim[0]; p.map_dim[1] = h->map_dim[1]; p.map_dim[2] = h->map_dim[2]; }
    p.width = h->width; p.height = h->height;
    if (setting_or(h, "hit_records", 1) != 0) {
        VRC_TRY(ensure_hits(h));
        p.hits = h->d_hits;
    }
    h->last_frame_wrote_hits = p.hits != nullptr;
    p.viewport = h->d_viewport; p.image = h->d_image;
    p.atlas = h->d_atlas; p.atlas_w = h->atlas_w; p.atlas_h = h->atlas_h;
    p.tiles_x = h->atlas_w / h->tile_w; p.tiles_y = h->atlas_h / h->tile_h;
    p.descriptors = t->d_desc;
    bind_attachments(t, p.attach_lookup, p.attachments);
    p.root_index = (uint64_t)root;
    // live buffers are re-read every frame (CL_MEM_USE_HOST_PTR semantics)
    for (int a = 0; a < 3; a++) p.cam_pos[a] = h->cam_pos[a];
    if (h->cam_trig) {                     // the host's own sin / cos (vrc_assign_camera_trig; ray_caster_kernel.cl:280-291)
        for (int a = 0; a < 4; a++) p.trig[a] = h->cam_trig[a];
    } else {
        p.trig[0] = sinf(h->cam_dir[0]); p.trig[1] = cosf(h->cam_dir[0]);
        p.trig[2] = sinf(h->cam_dir[1]); p.trig[3] = cosf(h->cam_dir[1]);
    }
    // the reference binds light_count but shades with light 0 only (ray_caster_kernel.cl:264,660-670); setting
    // "light_count" (default 1) switches on the multi-light extension for the first n packed lights
    p.light_count = (int32_t)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(setting_or(h, "light_count", 1), *h->light_count),
                                                                    vrc::kMaxLights));
    double light_reach = 0.0;              // steps a shadow ray may take beyond max_distance: |voxel - light| (:667)
    for (int l = 0; l < p.light_count; l++) {
        for (int k = 0; k < 7; k++) p.lights[l][k] = h->lights[10 * l + k];
        p.lights[l][7] = 0.0f;
        double far2 = 0.0;
        for (int a = 0; a < 3; a++) {
            const double lo = std::fabs((double)p.lights[l][4 + a]), hi = std::fabs((double)p.lights[l][4 + a] - (double)p.map_dim[a]);
            far2 += std::max(lo, hi) * std::max(lo, hi);
        }
        light_reach += std::sqrt(far2) + 2.0;
    }
    {   // the kernel's step counter is the reference's int (:325): a cap beyond 2^30 would overflow it on the way
        const int64_t md = setting_or(h, "max_distance", 20);
        if (md > (int64_t)1 << 30 || md < -((int64_t)1 << 30))
            return fail(h, VRC_ERR_INVALID_ARGUMENT, "compute: max_distance %lld is outside [-2^30, 2^30]", (long long)md);
        p.max_distance = (int32_t)md;
    }
    p.shadow_rays = (int32_t)setting_or(h, "shadow_rays", 1);
    // wave scheduling knobs of the SVO kernel; they never change results
    p.burst_steps = (int32_t)std::min<int64_t>(1 << 20, std::max<int64_t>(1, setting_or(h, "burst_steps", vrc::kDefaultBurstSteps)));
    p.shade_threshold = std::min<int64_t>(64, std::max<int64_t>(1, setting_or(h, "shade_threshold", vrc::kDefaultShadeThreshold)));

    p.widen_nodes = (int32_t)setting_or(h, "widen_nodes", 1);
    p.octree_bias = (int32_t)setting_or(h, "octree_bias", 1);
    p.arith_mask = (int32_t)setting_or(h, "arith_mask", 1);
    // every round advances at least one lane by a step, an event or a hit block: 64 lanes x (the longest legal ray:
    // max_distance primary steps + per light the distance to the farthest map corner) with a 2x margin
    const double legal_steps = (double)std::max(p.max_distance, 0) + light_reach + 64.0;
    p.watchdog_rounds = (int32_t)std::min<int64_t>(INT32_MAX, std::max<int64_t>(1, setting_or(h, "watchdog_rounds",
                                    (int64_t)std::min(2.0e9, 128.0 * legal_steps))));
    p.watchdog_flag = h->wd_flag;
    p.safe_run = (int32_t)setting_or(h, "safe_run", 1);
    p.single_step = (int32_t)setting_or(h, "single_step", 1);
    p.exact_steps = (int32_t)std::min<int64_t>(1 << 20, std::max<int64_t>(1, setting_or(h, "exact_steps", vrc::kDefaultExactSteps)));
    p.xcd_mode = (int32_t)setting_or(h, "xcd_mode", 1);
    p.lds_pad_bytes = (int32_t)std::min<int64_t>(120 * 1024, std::max<int64_t>(0, setting_or(h, "lds_pad_bytes", 0)));
    p.frame = h->d_frame;

    const int tile_rows = (h->height + vrc::kTileH - 1) / vrc::kTileH;
    p.band_tiles = h->band_rows / vrc::kTileH;
    p.tile_rank = h->tile_rank; p.tile_world = h->tile_world;
    p.row_sliced = h->sliced ? 1 : 0;
    const int bands = (tile_rows + p.band_tiles - 1) / p.band_tiles;
    int local_rows = 0;
    for (int b = h->tile_rank; b < bands; b += h->tile_world) {
        const int first = b * p.band_tiles;
        local_rows += std::min(p.band_tiles, tile_rows - first);
    }
    p.local_tile_rows = local_rows;
    p.blocks_x = (h->width + vrc::kTileW * vrc::kTilesPerBlock - 1) / (vrc::kTileW * vrc::kTilesPerBlock);
    // What the kernels derive from the tree (the dense table of its top, the empty boxes) lives WITH the tree and is built by
    // vrc_prepare / vrc_validate; a frame that finds it missing or built for other settings builds it here (under the guard).
    if (svo) derive_from_tree(h, t, p.log2_dim, p.root_index, p.stepping_mode, p);
    // exact closed-form jumps: on from depth 12; the threshold depends on where the Euclid tables live (LDS when stack + tables
    // fit at full occupancy: depth 12)
    p.jump_tables_lds = (int32_t)std::min<int64_t>(2, std::max<int64_t>(0, setting_or(h, "jump_tables_lds", 2)));
    const int lds_rows = vrc::jump_tables_lds_rows(p);             // 3, 2 (deep trees with boxes) or 0 rows of the tables' ring in LDS
    const bool tables_in_lds = lds_rows > 0;
    p.jump_tables_lds = lds_rows;                                  // resolved once, here: the launch takes it as it is
    // (the jump instances read the tree's top from the coarse table: without one -- depth < 5, coarse_log2 = 0 -- there are no jumps)
    p.jump_min_run = !p.coarse ? vrc::kJumpOff : (int32_t)std::min<int64_t>(vrc::kJumpOff, std::max<int64_t>(1, setting_or(h, "jump_min_run",
                                    p.log2_dim >= (p.boxes ? vrc::kDefaultJumpMinDepthBoxes : vrc::kDefaultJumpMinDepth) ? (tables_in_lds ? vrc::kDefaultJumpMinRunLds : vrc::kDefaultJumpMinRun)
                                                                            : vrc::kJumpOff)));
    p.safe_steps = (int32_t)std::min<int64_t>(256, std::max<int64_t>(2, setting_or(h, "safe_steps",
                                    p.jump_min_run < vrc::kJumpOff ? vrc::kDefaultSafeStepsJump : vrc::kDefaultSafeSteps)));
    // one row of counter partials per WORKGROUP of the kernel that will run (the exact SVO kernel's are finer than a 4-tile block:
    // vrc_params.h svo_tiles_per_workgroup), known now that the instance is: the partials, the reduction and the table slots follow it
    const int nblocks = vrc::raycast_workgroups(p), wg_tiles = vrc::raycast_workgroup_tiles(p);
    if (nblocks > h->partial_blocks) {
        release(h->d_partials);
        h->partial_blocks = 0;
        HIP_TRY(h, hipMalloc((void **)&h->d_partials, sizeof(unsigned long long) * vrc::kCtrCount * (size_t)nblocks));
        h->partial_blocks = nblocks;
    }
    p.counters = h->d_partials;
    if (svo && p.stepping_mode == 0 && p.jump_min_run < vrc::kJumpOff && !tables_in_lds) {
        VRC_TRY(ensure_jump_cache(h, nblocks, wg_tiles));
        p.jump_cache = h->d_jump_cache; p.jump_slots = h->d_jump_slots; p.jump_slot_count = h->jump_slot_count;
    }
    h->last_frame_boxes = p.boxes != nullptr;
    h->last_blocks = nblocks;
    h->frames_enqueued++;

    vrc_caster::EvPair ev;
    if (!h->pool.empty()) { ev = h->pool.back(); h->pool.pop_back(); }
    else { HIP_TRY(h, hipEventCreate(&ev.a)); HIP_TRY(h, hipEventCreate(&ev.b)); }

#ifdef VRC_INDEX_AUDIT
    {   // every array this frame's kernels may index (the launchers add the dynamic LDS): a null pointer's array is published empty
        using namespace vrc::audit;
        AuditExtents x;
        const size_t npix = (size_t)h->width * (size_t)std::max(h->buffer_rows, 1);
        audit_tree(x, t);
        x.set(kViewport, npix); x.set(kImage, npix); x.set(kHits, p.hits ? 2 * npix : 0);
        x.set(kAtlas, (size_t)h->atlas_w * h->atlas_h);
        x.set(kMap, h->d_map ? (size_t)h->map_dim[0] * h->map_dim[1] * h->map_dim[2] : 0);
        x.set(kPartials, (size_t)nblocks * vrc::kCtrCount); x.set(kCounters, vrc::kCtrCount); x.set(kFrame, 4);
        x.set(kJumpCache, p.jump_cache ? (size_t)h->jump_slot_count * h->jump_slot_threads * vrc::kJumpTableDwordsPerLane / 2 : 0);
        x.set(kJumpSlots, p.jump_slots ? (size_t)h->jump_slot_count : 0);
        VRC_AUDIT_PUBLISH(h, x);
    }
#endif
    HIP_TRY(h, vrc::launch_frame_setup(p, h->stream));
    HIP_TRY(h, hipEventRecord(ev.a, h->stream));
    HIP_TRY(h, vrc::launch_raycast(p, h->stream, &h->last_launch));
    HIP_TRY(h, hipEventRecord(ev.b, h->stream));
    h->pending.push_back(ev);
    if (h->pending.size() > 4096) { HIP_TRY(h, hipStreamSynchronize(h->stream)); drain_events(h); }
    return VRC_OK;
}

// what read_image / read_hits / read_image_rgba8 have in common: every rank copies its rows into the caller's frame
// (asynchronously, each on its own stream), then all ranks are waited for
// A group reading into pageable memory stages every rank's tile through its own pinned buffer, so that the n copies
// still run side by side (a pageable hipMemcpyAsync blocks the host thread); a single handle copies directly.
template <class Enqueue>
int gather_rows(vrc_caster *h, void *host, size_t bpp, Enqueue enqueue) {
    const bool stage = !h->peers.empty() && !host_is_pinned(host, bpp * (size_t)h->width * (size_t)h->height);
    int rc = enqueue(h, stage);
    if (rc != VRC_OK) return rc;
    for (size_t i = 0; i < h->peers.size(); i++) {
        rc = enqueue(h->peers[i], stage);
        if (rc != VRC_OK) return fail(h, rc, "rank %zu: %s", i + 1, h->peers[i]->error.c_str());
    }
    rc = sync_one(h);
    if (rc != VRC_OK) return rc;
    if (stage) finish_rows_out(h, bpp, host);
    for (size_t pi = 0; pi < h->peers.size(); pi++) {
        vrc_caster *q = h->peers[pi];
        rc = sync_one(q);
        if (rc != VRC_OK) return fail(h, rc, "rank %zu: %s", pi + 1, q->error.c_str());
        if (stage) finish_rows_out(q, bpp, host);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    return VRC_OK;
}

}  // namespace

extern "C" {

int vrc_compute_async(vrc_caster *h) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    VRC_TRY(compute_async_one(h));
    FOR_PEERS(h, compute_async_one(q));
    if (!h->peers.empty()) HIP_TRY(h, hipSetDevice(h->device));
    return VRC_OK;
}

int vrc_sync(vrc_caster *h) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int rc = sync_one(h);
    for (size_t i = 0; i < h->peers.size(); i++) {                 // always wait for every rank, then report the first failure
        const int rq = sync_one(h->peers[i]);
        if (rq != VRC_OK && rc == VRC_OK) rc = fail(h, rq, "rank %zu: %s", i + 1, h->peers[i]->error.c_str());
    }
    if (!h->peers.empty()) (void)hipSetDevice(h->device);
    return rc;
}

int vrc_compute(vrc_caster *h) {
    int rc = vrc_compute_async(h);
    if (rc != VRC_OK) return rc;
    return vrc_sync(h);                    // clFinish (CLCaster.cpp:970): the frame is complete on every rank
}

int vrc_read_image_f32(vrc_caster *h, float *rgba, size_t n_floats) {
    if (!h || !rgba) return VRC_ERR_INVALID_ARGUMENT;
    if (!h->d_image) return fail(h, VRC_ERR_NOT_READY, "read_image: no viewport");
    if (n_floats < (size_t)4 * h->width * h->height) return fail(h, VRC_ERR_INVALID_ARGUMENT, "read_image_f32: buffer too small");
    return gather_rows(h, rgba, 16, [rgba](vrc_caster *q, bool stage) -> int {
        HIP_TRY(q, hipSetDevice(q->device));
        return copy_rows_out(q, q->d_image, 16, rgba, stage);
    });
}

// CLCaster::draw's source (CLCaster.cpp:278-296,330-332) is an RGBA8 texture the kernel's write_imagef quantises into:
// saturate, scale by 255, round to nearest even.  Packed on the device, 4 bytes per pixel cross PCIe.
int vrc_read_image_rgba8(vrc_caster *h, uint8_t *rgba, size_t n_bytes) {
    if (!h || !rgba) return VRC_ERR_INVALID_ARGUMENT;
    if (!h->d_image) return fail(h, VRC_ERR_NOT_READY, "read_image: no viewport");
    if (n_bytes < (size_t)4 * h->width * h->height) return fail(h, VRC_ERR_INVALID_ARGUMENT, "read_image_rgba8: buffer too small");
    return gather_rows(h, rgba, 4, [rgba](vrc_caster *q, bool stage) -> int {
        HIP_TRY(q, hipSetDevice(q->device));
        const size_t npix = (size_t)q->width * (size_t)std::max(q->buffer_rows, 1);
        if (!q->d_rgba8) HIP_TRY(q, hipMalloc((void **)&q->d_rgba8, 4 * npix));
#ifdef VRC_INDEX_AUDIT
        { AuditExtents x; x.set(vrc::audit::kImage, npix); x.set(vrc::audit::kRgba8, npix); VRC_AUDIT_PUBLISH(q, x); }
#endif
        HIP_TRY(q, vrc::launch_pack_rgba8(q->d_image, q->d_rgba8, npix, q->stream));
        return copy_rows_out(q, q->d_rgba8, 4, rgba, stage);
    });
}

int vrc_read_hits(vrc_caster *h, int32_t *hits, size_t n_int32) {
    if (!h || !hits) return VRC_ERR_INVALID_ARGUMENT;
    if (!h->d_viewport) return fail(h, VRC_ERR_NOT_READY, "read_hits: no viewport");
    // the records must belong to the frame the image belongs to: with hit_records switched off since, the buffer still
    // holds an older frame's records
    if (!h->d_hits || !h->last_frame_wrote_hits)
        return fail(h, VRC_ERR_NOT_READY, "read_hits: no hit records (setting hit_records is 0, or no frame computed yet)");
    if (n_int32 < (size_t)8 * h->width * h->height) return fail(h, VRC_ERR_INVALID_ARGUMENT, "read_hits: buffer too small");
    return gather_rows(h, hits, 32, [hits](vrc_caster *q, bool stage) -> int {
        HIP_TRY(q, hipSetDevice(q->device));
        if (!q->d_hits || !q->last_frame_wrote_hits) return fail(q, VRC_ERR_NOT_READY, "read_hits: no hit records");
        return copy_rows_out(q, q->d_hits, 32, hits, stage);
    });
}

int vrc_device_image(vrc_caster *h, void **dev_ptr, size_t *n_bytes) {
    if (!h || !dev_ptr) return VRC_ERR_INVALID_ARGUMENT;
    if (!h->d_image) return fail(h, VRC_ERR_NOT_READY, "device_image: no viewport");
    *dev_ptr = h->d_image;
    if (n_bytes) *n_bytes = (size_t)16 * h->width * (size_t)h->buffer_rows;
    return VRC_OK;
}

int vrc_pin_host_buffer(void *p, size_t bytes) {
    if (!p || !bytes) return VRC_ERR_INVALID_ARGUMENT;
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) return VRC_OK;
    (void)hipGetLastError();
    return VRC_ERR_DEVICE;
}
int vrc_unpin_host_buffer(void *p) {
    if (!p) return VRC_ERR_INVALID_ARGUMENT;
    if (hipHostUnregister(p) == hipSuccess) return VRC_OK;
    (void)hipGetLastError();                 // reported through the return code, not left behind for the next launch
    return VRC_ERR_DEVICE;
}

// self-check of the empty boxes the last frame used: pseudo-random voxels inside pseudo-random boxes, looked up in the tree
int vrc_empty_boxes_check(vrc_caster *h, uint64_t samples, uint64_t seed, uint64_t *boxes_sampled, uint64_t *solid_voxels, double *build_seconds) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    vrc_tree *t = h->tree.get();
    if (!t) return fail(h, VRC_ERR_NOT_READY, "empty_boxes_check: no octree");
    std::lock_guard<std::mutex> lock(t->guard);
    if (!t->d_box_aux || !t->d_desc) return fail(h, VRC_ERR_NOT_READY, "empty_boxes_check: no boxes (setting empty_boxes, or neither vrc_prepare nor a frame has run yet)");
    HIP_TRY(h, hipSetDevice(h->device));
    uint64_t *pos = nullptr; unsigned long long *res = nullptr;
    hipError_t e = hipMalloc((void **)&res, 2 * sizeof(unsigned long long));
    unsigned long long out[2] = {0, 0}, cells[2] = {0, 0};
    const TableKey &at = t->boxes.built.at;
#ifdef VRC_INDEX_AUDIT
    if (e == hipSuccess) {   // the tree and its boxes; the positions and descriptor indices of the records the check samples
        AuditExtents x;
        audit_tree(x, t);
        x.set(vrc::audit::kBoxPos, t->boxes.built.mode == 2 ? t->box_records : t->n_desc);
        x.set(vrc::audit::kBoxDesc, t->boxes.built.mode == 2 ? t->box_records : 0);
        e = audit_publish(x);
    }
#endif
    if (t->d_boxes && t->boxes.built.mode == 2) {              // the records of the upper levels (their descriptors and positions were kept)
        if (e == hipSuccess) e = vrc::launch_box_check(t->d_desc, t->box_records, at.root, at.depth, t->d_box_pos, t->d_box_desc, t->d_boxes, samples, seed, res, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) e = hipMemcpy(out, res, sizeof(out), hipMemcpyDeviceToHost);
    } else if (t->d_boxes) {                                   // the words per (descriptor, child)
        if (e == hipSuccess) e = hipMalloc((void **)&pos, sizeof(uint64_t) * t->n_desc);
        if (e == hipSuccess) e = vrc::launch_box_positions(t->d_desc, t->n_desc, at.root, at.depth, pos, h->stream);
        if (e == hipSuccess) e = vrc::launch_box_check(t->d_desc, t->n_desc, at.root, at.depth, pos, nullptr, t->d_boxes, samples, seed, res, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) e = hipMemcpy(out, res, sizeof(out), hipMemcpyDeviceToHost);
    }
    // the words of the table's cells (the coarse space)
    if (e == hipSuccess) e = vrc::launch_box_check_cells(t->d_desc, at.root, at.depth, at.log2, t->d_box_aux, samples, seed + 1, res, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipMemcpy(cells, res, sizeof(cells), hipMemcpyDeviceToHost);
    out[0] += cells[0]; out[1] += cells[1];
    if (pos) (void)hipFree(pos);
    if (res) (void)hipFree(res);
    HIP_TRY(h, e);
    if (boxes_sampled) *boxes_sampled = out[0];
    if (solid_voxels) *solid_voxels = out[1];
    if (build_seconds) *build_seconds = t->box_build_seconds;
    return VRC_OK;
}

// read-back of the box words (tests: every voxel of every box of a small tree against its dense grid, on the host)
int vrc_read_empty_boxes(vrc_caster *h, uint64_t first_descriptor, uint64_t count, uint32_t *out) {
    if (!h || !out) return VRC_ERR_INVALID_ARGUMENT;
    vrc_tree *t = h->tree.get();
    if (!t) return fail(h, VRC_ERR_NOT_READY, "read_empty_boxes: no octree");
    std::lock_guard<std::mutex> lock(t->guard);
    if (!t->d_boxes) return fail(h, VRC_ERR_NOT_READY, "read_empty_boxes: no boxes (setting empty_boxes, or neither vrc_prepare nor a frame has run yet)");
    if (t->boxes.built.mode != 1) return fail(h, VRC_ERR_NOT_READY, "read_empty_boxes: this tree has box records for its upper levels only (they are not indexed by descriptor)");
    if (first_descriptor > t->n_desc || count > t->n_desc - first_descriptor) return fail(h, VRC_ERR_INVALID_ARGUMENT, "read_empty_boxes: range past the array");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpy(out, t->d_boxes + 8 * first_descriptor, sizeof(uint32_t) * 8 * count, hipMemcpyDeviceToHost));
    return VRC_OK;
}

// vrc_memory_usage with a size-versioned struct (the caller says how large ITS struct is; never more than that is written)
int vrc_memory_usage2(vrc_caster *h, int32_t rank, vrc_memory2 *out) {
    if (!h || !out || rank < 0 || rank > (int32_t)h->peers.size() || out->struct_size < sizeof(uint32_t)) return VRC_ERR_INVALID_ARGUMENT;
    const vrc_caster *q = rank == 0 ? h : h->peers[rank - 1];
    vrc_memory2 m;
    memset(&m, 0, sizeof(m));
    const size_t npix = q->d_viewport ? (size_t)q->width * (size_t)std::max(q->buffer_rows, 1) : 0;
    m.device = q->device; m.rows = q->buffer_rows;
    m.viewport_bytes = 16 * npix; m.image_bytes = 16 * npix; m.hit_bytes = q->d_hits ? 32 * npix : 0;
    m.octree_shared = q->owns_desc ? 0 : 1;
    m.peer_access = q->peer_access;
    if (const vrc_tree *t = q->tree.get()) {
        // (what is allocated: after an edit has grown the arrays, more than the n_desc words vrc_octree_size reports)
        m.octree_bytes = t->desc_capacity() * 8 + (t->d_attach_lookup ? t->lookup_capacity() * 4 + t->attach_capacity() * 8 : 0);
        m.tree_holders = (int32_t)q->tree.use_count();
        m.coarse_log2 = t->d_coarse ? t->coarse.built.log2 : 0;
        m.coarse_bytes = t->d_coarse ? (uint64_t)sizeof(uint64_t) << (3 * t->coarse.built.log2) : 0;
        m.empty_boxes = q->last_frame_boxes ? 1 : 0;
        m.box_bytes = (t->d_boxes ? (uint64_t)t->box_records * (32 + (t->boxes.built.mode == 2 ? 20 : 0)) : 0) +
                      (t->d_box_aux ? (uint64_t)sizeof(uint32_t) << (3 * t->boxes.built.at.log2) : 0);
        m.box_records = t->d_boxes ? t->box_records : 0;
        m.box_levels = t->d_boxes ? t->box_levels : 0;
        m.box_build_seconds = t->box_build_seconds;
        snprintf(m.note, sizeof(m.note), "%s%s", t->coarse.note.c_str(), t->boxes.note.c_str());
        m.box_queries_cut = t->d_boxes ? t->box_queries_cut : 0;
    }
    write_info(out, m);
    return VRC_OK;
}

// the older, fixed struct: the fields it shares with vrc_memory2
int vrc_memory_usage(vrc_caster *h, int32_t rank, vrc_memory *out) {
    if (!out) return VRC_ERR_INVALID_ARGUMENT;
    vrc_memory2 m;
    m.struct_size = sizeof(m);
    VRC_TRY(vrc_memory_usage2(h, rank, &m));
    memset(out, 0, sizeof(*out));
    out->device = m.device; out->rows = m.rows;
    out->viewport_bytes = m.viewport_bytes; out->image_bytes = m.image_bytes; out->hit_bytes = m.hit_bytes; out->octree_bytes = m.octree_bytes;
    out->octree_shared = m.octree_shared; out->peer_access = m.peer_access;
    out->coarse_bytes = m.coarse_bytes;
    return VRC_OK;
}

}  // extern "C"

namespace {
int counters_one(vrc_caster *h, unsigned long long c[vrc::kCtrCount]) {
    if (h->frames_enqueued && h->last_blocks == 0) {             // a rank that owns no rows of this frame (more ranks than bands)
        memset(c, 0, sizeof(unsigned long long) * vrc::kCtrCount);
        return VRC_OK;
    }
    if (!h->d_partials || h->last_blocks <= 0) return fail(h, VRC_ERR_NOT_READY, "get_counters: no frame computed");
    HIP_TRY(h, hipSetDevice(h->device));
#ifdef VRC_INDEX_AUDIT
    { AuditExtents x; x.set(vrc::audit::kPartials, (size_t)h->last_blocks * vrc::kCtrCount); x.set(vrc::audit::kCounters, vrc::kCtrCount); VRC_AUDIT_PUBLISH(h, x); }
#endif
    HIP_TRY(h, vrc::launch_reduce_counters(h->d_partials, h->last_blocks, h->d_counters, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(c, h->d_counters, sizeof(unsigned long long) * vrc::kCtrCount, hipMemcpyDeviceToHost));
    return VRC_OK;
}
}  // namespace

extern "C" {

int vrc_get_counters(vrc_caster *h, vrc_counters *out) {
    if (!h || !out) return VRC_ERR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    unsigned long long c[vrc::kCtrCount], t[vrc::kCtrCount];
    int rc = counters_one(h, c);
    if (rc != VRC_OK) return rc;
    for (size_t i = 0; i < h->peers.size(); i++) {                 // a group reports the whole frame
        rc = counters_one(h->peers[i], t);
        if (rc != VRC_OK) return fail(h, rc, "rank %zu: %s", i + 1, h->peers[i]->error.c_str());
        for (int k = 0; k < vrc::kCtrCount; k++) c[k] += t[k];
    }
    if (!h->peers.empty()) HIP_TRY(h, hipSetDevice(h->device));
    out->primary_rays = c[vrc::kCtrPrimary]; out->shadow_rays = c[vrc::kCtrShadow];
    out->descriptor_reads = c[vrc::kCtrDesc]; out->texel_reads = c[vrc::kCtrTex];
    out->map_reads = c[vrc::kCtrMap]; out->steps = c[vrc::kCtrSteps];
    out->unwritten_pixels = c[vrc::kCtrUnwritten];
    out->watchdog_trips = c[vrc::kCtrWatchdog];
    for (int i = 0; i < 8; i++) h->sched_stats[i] = c[8 + i];
    if (out->watchdog_trips)
        return fail(h, VRC_ERR_DEVICE, "the kernel's round watchdog stopped %llu wavefronts: the frame is invalid",
                    (unsigned long long)out->watchdog_trips);
    return VRC_OK;
}

int vrc_counters_canonical(vrc_caster *h, int32_t *canonical) {
    if (!h || !canonical) return VRC_ERR_INVALID_ARGUMENT;
    bool boxes = h->last_frame_boxes;
    for (const vrc_caster *q : h->peers) boxes = boxes || q->last_frame_boxes;
    *canonical = boxes ? 0 : 1;
    return VRC_OK;
}

// what launch_raycast recorded for the rank's last enqueued frame, size-versioned like vrc_memory_usage2
int vrc_last_kernel(vrc_caster *h, int32_t rank, vrc_kernel_info *out) {
    if (!h || !out || rank < 0 || rank > (int32_t)h->peers.size() || out->struct_size < sizeof(uint32_t)) return VRC_ERR_INVALID_ARGUMENT;
    const vrc_caster *q = rank == 0 ? h : h->peers[rank - 1];
    if (!q->frames_enqueued) return fail(h, VRC_ERR_NOT_READY, "last_kernel: no frame computed");
    const vrc::LaunchRecord &r = q->last_launch;
    vrc_kernel_info k;
    memset(&k, 0, sizeof(k));
    k.family = r.family; k.n_args = r.n_args;
    for (int i = 0; i < 6; i++) k.args[i] = i < r.n_args ? r.args[i] : -1;
    k.jump_min_run = r.jump_min_run; k.lds_rows = r.lds_rows;
    static const char *const family[] = {"", "raycast_svo_kernel", "raycast_jump_kernel", "raycast_array_kernel"};
    std::string name = family[r.family];
    for (int i = 0; i < r.n_args; i++) {
        name += i ? ", " : "<";
        name += ((r.int_args >> i) & 1) ? std::to_string(r.args[i]) : std::string(r.args[i] ? "true" : "false");
    }
    if (r.n_args) name += ">";
    snprintf(k.name, sizeof(k.name), "%s", name.c_str());
    const uint32_t n = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof(k));
    k.struct_size = n;
    memcpy(out, &k, n);
    return VRC_OK;
}

// the index audit's report and its test-only knob (include/vrc.h); the product build has neither
int vrc_index_audit_report(int32_t device, vrc_index_audit_entry *out, int32_t n_entries, int32_t clear) {
#ifdef VRC_INDEX_AUDIT
    static_assert(VRC_AUDIT_ARRAYS == vrc::audit::kArrayCount, "include/vrc.h states the number of audited arrays");
    if (!out || n_entries < 0 || n_entries > VRC_AUDIT_ARRAYS) return VRC_ERR_INVALID_ARGUMENT;
    DeviceRestore restore;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return VRC_ERR_INVALID_ARGUMENT; }
    vrc::audit::Stat sum[vrc::audit::kArrayCount];
    memset(sum, 0, sizeof(sum));
    unsigned long long e1[vrc::audit::kArrayCount] = {};             // the extent the accessed array was last checked against
    hipError_t e = hipDeviceSynchronize();
    for (const AuditTu &tu : kAuditTus)
        if (e == hipSuccess) e = tu.collect(sum, e1, clear);
    if (e != hipSuccess) { (void)hipGetLastError(); return VRC_ERR_DEVICE; }
    for (int i = 0; i < n_entries; i++) {
        vrc_index_audit_entry &o = out[i];
        memset(&o, 0, sizeof(o));
        o.accesses = sum[i].accesses; o.max_index = sum[i].max_index; o.violations = sum[i].violations;
        o.extent_published = e1[i] != 0; o.extent = e1[i] ? e1[i] - 1 : 0;
        o.first_index = sum[i].first_index; o.first_extent = sum[i].first_extent; o.first_block = sum[i].first_block; o.first_site = sum[i].first_site;
    }
    return VRC_OK;
#else
    (void)device; (void)out; (void)n_entries; (void)clear;
    return VRC_ERR_NOT_READY;
#endif
}

int vrc_index_audit_shrink(int32_t array_id, uint64_t amount) {
#ifdef VRC_INDEX_AUDIT
    if (array_id < 0 || array_id >= vrc::audit::kArrayCount) return VRC_ERR_INVALID_ARGUMENT;
    g_audit_shrink[array_id] = amount;
    return VRC_OK;
#else
    (void)array_id; (void)amount;
    return VRC_ERR_NOT_READY;
#endif
}

int vrc_get_scheduler_stats(vrc_caster *h, uint64_t out[8]) {
    if (!h || !out) return VRC_ERR_INVALID_ARGUMENT;
    vrc_counters tmp;
    int rc = vrc_get_counters(h, &tmp);
    if (rc != VRC_OK) return rc;
    for (int i = 0; i < 8; i++) out[i] = h->sched_stats[i];
    return VRC_OK;
}

int vrc_timing_reset(vrc_caster *h) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int rc = vrc_sync(h);
    h->timed_launches = 0; h->timed_ms = 0.0;
    for (vrc_caster *q : h->peers) { q->timed_launches = 0; q->timed_ms = 0.0; }
    return rc;
}

// a group reports rank 0's launch count and the largest per-rank kernel time (the critical path of the frame)
int vrc_timing_get(vrc_caster *h, uint64_t *n_launches, double *total_kernel_ms) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int rc = vrc_sync(h);
    double ms = h->timed_ms;
    for (vrc_caster *q : h->peers) ms = std::max(ms, q->timed_ms);
    if (n_launches) *n_launches = h->timed_launches;
    if (total_kernel_ms) *total_kernel_ms = ms;
    return rc;
}

}  // extern "C"
