// vrc_scene_edit.cpp -- the calls of include/vrc.h that change the resident scene: point edits (vrc_set_voxels, voxel_edit.hip),
// region edits (vrc_fill_boxes / vrc_write_regions / vrc_fill_shapes, region_write.hip) and the compaction of the octree (vrc_compact_octree,
// octree_compact.hip), with their _device variants.
//
// They are one procedure.  On every rank of the group (run_group) a STAGE takes the tree's guard, drains the stream and binds the
// scene without its coarse table (stage_begin), runs its kernels in timed segments, each ended by the read-back that sizes the
// next one (SegmentTimer), and leaves new arrays beside the tree's where the old ones have no room (stage_array).  Until then the
// tree is what it was.  Then every rank commits (edit_commit), every rank's root moves, and the call's info struct is written.
#include "octree_compact.h"
#include "region_write.h"
#include "shape_span.hpp"
#include "voxel_edit.h"
#include "vrc_host.hpp"

namespace {

std::vector<vrc_caster *> group_of(vrc_caster *h) {
    std::vector<vrc_caster *> group{h};
    group.insert(group.end(), h->peers.begin(), h->peers.end());
    return group;
}

// a holder of the tree outside this group would keep rendering from the old root: its setting cannot be moved from here
int group_alone_holds_trees(vrc_caster *h, const char *what) {
    const std::vector<vrc_caster *> group = group_of(h);
    for (const vrc_caster *g : group) {
        if (!g->tree) return fail(h, VRC_ERR_NOT_READY, "%s: a rank of the group has no octree", what);
        long inside = 0;
        for (const vrc_caster *o : group) inside += o->tree.get() == g->tree.get() ? 1 : 0;
        if (g->tree.use_count() > inside)
            return fail(h, VRC_ERR_LIMIT, "%s: the tree is also held by a handle outside this group (vrc_assign_octree_from); its root cannot be moved from here", what);
    }
    return VRC_OK;
}

// What one handle's call has prepared and edit_commit installs.  Until then the tree is what it was: the appended words lie
// behind n_desc, in the tree's own arrays where they had room and in the arrays staged here where they had not.
struct EditStage {
    vrc_caster *h = nullptr;
    bool ran = false, commit = false;
    int64_t skipped = 0, changed = 0, bricks = 0;
    uint64_t added = 0, n_desc = 0, root = 0, n_attach = 0;
    double seconds = 0.0;
    uint64_t *desc = nullptr; uint32_t *lookup = nullptr; uint64_t *attach = nullptr;       // replace the tree's at the commit
    uint64_t cap_desc = 0, cap_lookup = 0, cap_attach = 0;
    EditStage() = default;
    EditStage(const EditStage &) = delete;
    EditStage &operator=(const EditStage &) = delete;
    ~EditStage() {
        if (!desc && !lookup && !attach) return;
        DeviceRestore restore;
        (void)hipSetDevice(h->device);
        release(desc); release(lookup); release(attach);
        (void)hipGetLastError();
    }
};

// What every stage opens with (current device: g->device): the tree's guard, which stays with the caller's lock; a frame in
// flight finishes first; the scene without its table (the table goes with the edit: every descent starts at the root); the timer.
// counters: where the edits want their counters, allocated on first use.
int stage_begin(vrc_caster *g, EditStage &st, std::unique_lock<std::mutex> &lock, SegmentTimer &timer, vrc::SceneView &scene,
                unsigned long long **counters = nullptr) {
    st.h = g; st.ran = true;
    lock = std::unique_lock<std::mutex>(g->tree->guard);
    HIP_TRY(g, hipStreamSynchronize(g->stream));
    bind_scene(g, g->tree.get(), scene);
    scene.coarse = nullptr; scene.coarse_log2 = 0;
    HIP_TRY(g, timer.init(g->stream, &st.seconds));
    if (counters && !g->d_edit_counters) HIP_TRY(g, hipMalloc((void **)&g->d_edit_counters, sizeof(unsigned long long) * vrc::kEditCounters));
    if (counters) *counters = g->d_edit_counters;
    return VRC_OK;
}

// The n keys of a batch, sorted (stable: equal keys stay in edit order) with their edit numbers beside them and, with `runs`, the
// unique keys and their run lengths.  Opens a timed segment with write_keys, the kernel that fills q.keys / q.order, and leaves
// the segment open: the caller adds to it and ends it.
template <class Launch>
int sort_keys(vrc_caster *g, vrc::EditParams &q, int64_t n, int bits, bool runs, SegmentTimer &timer, Launch write_keys) {
    VRC_TRY(grow(g, g->edit_capacity, n, {{g->d_edit_keys, sizeof(uint64_t) * 2 * (size_t)n}, {g->d_edit_order, sizeof(uint32_t) * 2 * (size_t)n},
                                    {g->d_edit_unique, sizeof(uint64_t) * (size_t)n}, {g->d_edit_counts, sizeof(uint32_t) * (size_t)n}}));
    q.n = n;
    q.keys = g->d_edit_keys; q.order = g->d_edit_order;
    q.sorted_keys = g->d_edit_keys + n; q.sorted_order = g->d_edit_order + n;
    unsigned long long *n_runs = q.counters + vrc::kEditRuns;
    size_t sort_bytes = 0, run_bytes = 0;
    HIP_TRY(g, vrc::edit_sort(nullptr, &sort_bytes, q.keys, g->d_edit_keys + n, q.order, g->d_edit_order + n, n, bits, g->stream));
    HIP_TRY(g, vrc::edit_runs(nullptr, &run_bytes, q.sorted_keys, n, g->d_edit_unique, g->d_edit_counts, n_runs, g->stream));
    const size_t temp_bytes = std::max<size_t>(std::max(sort_bytes, run_bytes), 16);
    VRC_TRY(grow(g, g->edit_temp_bytes, temp_bytes, {{g->d_edit_temp, temp_bytes}}));
    HIP_TRY(g, timer.start());
    HIP_TRY(g, write_keys());
    HIP_TRY(g, vrc::edit_sort(g->d_edit_temp, &sort_bytes, q.keys, g->d_edit_keys + n, q.order, g->d_edit_order + n, n, bits, g->stream));
    if (runs) HIP_TRY(g, vrc::edit_runs(g->d_edit_temp, &run_bytes, q.sorted_keys, n, g->d_edit_unique, g->d_edit_counts, n_runs, g->stream));
    return VRC_OK;
}

// (asked once per stage, before its first array: the reserves of one call do not depend on each other)
size_t free_device_bytes() {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
    return free_b;
}

// A new tree array of `need` words beside the old one: the tree keeps its own until the commit.  Behind the words a reserve for the
// edits to come (setting edit_reserve; -1: an eighth of the need, at least 4096 words, at most a sixteenth of the free device memory)
template <class T>
int stage_array(vrc_caster *g, T *&p, uint64_t &cap, uint64_t need, size_t free_bytes, const char *what) {
    const int64_t asked = setting_or(g, "edit_reserve", -1);
    cap = need + (asked >= 0 ? (uint64_t)asked : std::min<uint64_t>(std::max<uint64_t>(need / 8, 4096), (uint64_t)(free_bytes / 16) / sizeof(T)));
    const hipError_t e = hipMalloc((void **)&p, cap * sizeof(T));
    if (e == hipSuccess) return VRC_OK;
    (void)hipGetLastError();
    p = nullptr;
    return fail(g, e == hipErrorOutOfMemory ? VRC_ERR_OUT_OF_MEMORY : VRC_ERR_DEVICE, "%s: allocating a new array of %llu words beside the old one failed: %s",
                what, (unsigned long long)need, hipGetErrorString(e));
}

// The last step: the staged arrays replace the tree's (the old ones are freed once the device is idle: hipFree waits), the
// appended words are taken, what was derived from the old tree goes, and the handle's root moves.
void edit_commit(EditStage &st) {
    vrc_caster *g = st.h;
    vrc_tree *t = g->tree.get();
    std::lock_guard<std::mutex> lock(t->guard);
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->stream);
    auto install = [](auto *&mine, auto *&staged, uint64_t &cap, uint64_t staged_cap) {
        if (!staged) return;
        auto *old = mine;
        mine = staged; cap = staged_cap; staged = nullptr;
        if (old) (void)hipFree(old);
    };
    install(t->d_desc, st.desc, t->cap_desc, st.cap_desc);
    install(t->d_attach_lookup, st.lookup, t->cap_lookup, st.cap_lookup);
    install(t->d_attach, st.attach, t->cap_attach, st.cap_attach);
    if (!t->cap_desc) t->cap_desc = t->n_desc;                        // (the capacities are what is allocated, from here on)
    if (t->d_attach_lookup && !t->cap_lookup) t->cap_lookup = t->n_desc;
    if (t->d_attach && !t->cap_attach) t->cap_attach = std::max<uint64_t>(t->n_attach, 1);
    t->n_desc = st.n_desc;
    if (st.n_attach) t->n_attach = st.n_attach;
    // the coarse table and the empty boxes describe the old tree: vrc_prepare / vrc_validate / the next frame build them again
    release(t->d_coarse); t->coarse.built = TableKey{};
    release_boxes(t);
    (void)hipGetLastError();
}

// Every rank of the group stages (stage_one(g, st), current device: g->device) -- but a rank that shares an earlier rank's tree has
// nothing to do; of the map (svo false) every rank has its own.  A peer's failure is reported through rank 0.  Then every stage that
// ran and asks for it commits, and every rank's root moves to rank 0's.
template <class Stage, class StageOne>
int run_group(vrc_caster *h, bool svo, std::vector<std::unique_ptr<Stage>> &stages, StageOne stage_one) {
    const std::vector<vrc_caster *> group = group_of(h);
    for (size_t r = 0; r < group.size(); r++) {
        vrc_caster *g = group[r];
        stages.emplace_back(new Stage());
        bool shared = false;
        for (size_t k = 0; k < r && svo; k++) shared = shared || group[k]->tree.get() == g->tree.get();
        if (shared) continue;
        HIP_TRY(h, hipSetDevice(g->device));
        const int rc = stage_one(g, *stages.back());
        if (rc != VRC_OK) return g == h ? rc : fail(h, rc, "rank %zu: %s", r, g->error.c_str());
    }
    if (svo && stages[0]->commit) {
        for (auto &st : stages)
            if (st->ran && st->commit) edit_commit(*st);
        for (vrc_caster *g : group) VRC_TRY(set_setting(g, "octree_root_index", "OCTREE_ROOT_INDEX", (int64_t)stages[0]->root));
    }
    HIP_TRY(h, hipSetDevice(h->device));
    return VRC_OK;
}

// What a call hands to every rank: its name, its two arrays -- positions (int32[3 n]) and materials (int32[n]); boxes (int32[6 n])
// and materials; corners (int32[3 n]) and blocks (n * volume bytes); shapes (int32[6 n]) and materials -- in host memory or in memory rank 0's GPU can read, and for
// the region edits what they do with them.
enum EditKind { kPoints = 0, kFill, kPaste, kShapes };
struct EditBatch {
    const char *what; const void *first, *second; int64_t n; bool on_device;
    EditKind kind; uint32_t flags; int32_t size[3] = {0, 0, 0}; uint64_t volume = 0;
    size_t first_bytes() const { return sizeof(int32_t) * (kind == kFill || kind == kShapes ? 6 : 3) * (size_t)n; }
    size_t second_bytes() const { return kind == kPaste ? (size_t)volume * (size_t)n : sizeof(int32_t) * (size_t)n; }
};

// What every front end of an SVO edit ends with (the tree's guard is held; q holds the scene, the sorted batch and the counters,
// d_unique the keys of the nb touched bricks in order, c the counters as read so far): size the appended range, make room,
// run the brick pass -- the region edits' own when `region` is given, which then takes q as its edit block -- and the ancestor
// pass of every level, and fill the stage for the commit.
int edit_append(vrc_caster *g, vrc::EditParams &q, vrc::RegionParams *region, int64_t nb, unsigned long long *c, SegmentTimer &timer, EditStage &st,
                const char *what) {
    vrc_tree *t = g->tree.get();
    const int nlog = q.scene.log2_dim, above = std::max(nlog - vrc::kReadBrickLog2, 0);   // levels above the bricks
    std::vector<std::vector<uint64_t>> levels((size_t)above);
    {
        std::vector<uint64_t> below((size_t)nb);
        HIP_TRY(g, hipMemcpy(below.data(), g->d_edit_unique, sizeof(uint64_t) * (size_t)nb, hipMemcpyDeviceToHost));
        for (int j = 0; j < above; j++) {
            std::vector<uint64_t> &here = levels[(size_t)j];
            for (uint64_t k : (j ? levels[(size_t)j - 1] : below))
                if (here.empty() || here.back() != k >> 3) here.push_back(k >> 3);
        }
    }
    int64_t ancestors = 0;
    for (const auto &l : levels) ancestors += (int64_t)l.size();
    // the appended range: [a root word in front of a depth-3 brick] the bricks, the levels from the bricks' parents up, the
    // root word in front of the root level's block
    const uint64_t first = t->n_desc;
    st.added = vrc::kEditBrickStride * (uint64_t)nb + vrc::kEditNodeStride * (uint64_t)ancestors + (nlog >= vrc::kReadBrickLog2 ? 1 : 0);
    st.bricks = nb;
    st.n_desc = first + st.added;
    q.brick_base = first + (nlog == vrc::kReadBrickLog2 ? 1 : 0);
    st.root = above ? st.n_desc - vrc::kEditNodeStride - 1 : first;
    const bool have = t->d_attach_lookup && t->d_attach, want = have || c[vrc::kEditMaterials] != 0;
    q.attach_base = have ? std::max<uint64_t>(t->n_attach, 1) : 1;    // (a tree that gets its materials now: slot 0 is eight 5s)
    st.n_attach = want ? q.attach_base + vrc::kEditBrickAttach * (uint64_t)nb : 0;
    if (st.n_attach > 0xffffffffULL) return fail(g, VRC_ERR_LIMIT, "%s: more than 2^32 attachment slots", what);
    if (st.n_desc >= (1ULL << 47)) return fail(g, VRC_ERR_LIMIT, "%s: more than 2^47 descriptors", what);

    // room: arrays that cannot take the batch are staged anew and copied device to device; the tree keeps its own until the commit
    const size_t free_b = free_device_bytes();
    if (st.n_desc > t->desc_capacity()) {
        VRC_TRY(stage_array(g, st.desc, st.cap_desc, st.n_desc, free_b, what));
        HIP_TRY(g, hipMemcpyAsync(st.desc, t->d_desc, first * sizeof(uint64_t), hipMemcpyDeviceToDevice, g->stream));
    }
    if (want && (!have || st.n_desc > t->lookup_capacity())) {
        VRC_TRY(stage_array(g, st.lookup, st.cap_lookup, st.n_desc, free_b, what));
        if (have) HIP_TRY(g, hipMemcpyAsync(st.lookup, t->d_attach_lookup, first * sizeof(uint32_t), hipMemcpyDeviceToDevice, g->stream));
        else HIP_TRY(g, hipMemsetAsync(st.lookup, 0, first * sizeof(uint32_t), g->stream));
    }
    if (want && (!have || st.n_attach > t->attach_capacity())) {
        VRC_TRY(stage_array(g, st.attach, st.cap_attach, st.n_attach, free_b, what));
        if (have) HIP_TRY(g, hipMemcpyAsync(st.attach, t->d_attach, q.attach_base * sizeof(uint64_t), hipMemcpyDeviceToDevice, g->stream));
        else HIP_TRY(g, hipMemsetAsync(st.attach, 0x05, sizeof(uint64_t), g->stream));
    }
    q.descriptors = st.desc ? st.desc : t->d_desc;
    q.attach_lookup = !want ? nullptr : st.lookup ? st.lookup : t->d_attach_lookup;
    q.attachments = !want ? nullptr : st.attach ? st.attach : t->d_attach;
    HIP_TRY(g, hipMemsetAsync(q.descriptors + first, 0, st.added * sizeof(uint64_t), g->stream));     // (what no pass stores stays zero)
    if (want) {
        HIP_TRY(g, hipMemsetAsync(q.attach_lookup + first, 0, st.added * sizeof(uint32_t), g->stream));
        HIP_TRY(g, hipMemsetAsync(q.attachments + q.attach_base, 0, (st.n_attach - q.attach_base) * sizeof(uint64_t), g->stream));
    }
    VRC_TRY(grow(g, g->edit_rec_capacity, nb + ancestors, {{g->d_edit_rec_masks, sizeof(uint32_t) * (size_t)(nb + ancestors)},
                                                     {g->d_edit_rec_child, sizeof(uint64_t) * (size_t)(nb + ancestors)}}));
    if (ancestors) VRC_TRY(grow(g, g->edit_level_capacity, ancestors, {{g->d_edit_levels, sizeof(uint64_t) * (size_t)ancestors}}));
    {
        int64_t at = 0;
        for (const auto &l : levels) {
            HIP_TRY(g, hipMemcpyAsync(g->d_edit_levels + at, l.data(), sizeof(uint64_t) * l.size(), hipMemcpyHostToDevice, g->stream));
            at += (int64_t)l.size();
        }
    }
    q.brick_keys = g->d_edit_unique; q.n_bricks = nb;
    q.rec_masks = g->d_edit_rec_masks; q.rec_child = g->d_edit_rec_child;
    HIP_TRY(g, timer.start());
    if (region) {
        region->edit = q;
        HIP_TRY(g, vrc::launch_region_bricks(*region, g->stream));
    } else {
        HIP_TRY(g, vrc::launch_edit_bricks(q, g->stream));
    }
    {
        vrc::EditLevel l;
        memset(&l, 0, sizeof(l));
        l.below_keys = g->d_edit_unique; l.below_count = nb; l.rec_below = 0;
        l.keys = g->d_edit_levels; l.rec_here = nb;
        l.base = first + vrc::kEditBrickStride * (uint64_t)nb;
        for (int j = 0; j < above; j++) {
            l.count = (int64_t)levels[(size_t)j].size();
            l.r = vrc::kReadBrickLog2 + 1 + j; l.root = j == above - 1 ? 1 : 0;
            HIP_TRY(g, vrc::launch_edit_level(q, l, g->stream));
            l.below_keys = l.keys; l.below_count = l.count; l.rec_below = l.rec_here;
            l.keys += l.count; l.rec_here += l.count; l.base += vrc::kEditNodeStride * (uint64_t)l.count;
        }
    }
    HIP_TRY(g, timer.end(c, q.counters, sizeof(unsigned long long) * vrc::kEditCounters));
    st.changed = (int64_t)c[vrc::kEditChanged];
    st.commit = st.changed != 0;              // a batch that changes no voxel appends nothing: the words behind n_desc are simply not taken
    return VRC_OK;
}

// One handle's edit up to the commit (current device: g->device; d_pos / d_mat: memory of that device).  The array branch
// stores in place; the SVO branch appends behind n_desc and leaves the commit to the caller.
int edit_stage(vrc_caster *g, const int32_t *d_pos, const int32_t *d_mat, int64_t n, EditStage &st) {
    vrc::EditParams q;
    memset(&q, 0, sizeof(q));
    std::unique_lock<std::mutex> lock;
    SegmentTimer timer;
    VRC_TRY(stage_begin(g, st, lock, timer, q.scene, &q.counters));
    const bool svo = q.scene.svo != 0;
    const int nlog = q.scene.log2_dim, above = std::max(nlog - vrc::kReadBrickLog2, 0);   // levels above the bricks
    int bits = 3 * above;
    if (!svo)
        for (bits = 0; bits < 63 && (1ULL << bits) <= q.scene.map_bytes; bits++) {}
    q.sentinel = svo ? 1ULL << bits : q.scene.map_bytes;
    q.positions = d_pos; q.materials = d_mat;
    q.map = g->d_map;
    unsigned long long c[vrc::kEditCounters];

    HIP_TRY(g, hipMemsetAsync(q.counters, 0, sizeof(c), g->stream));
    VRC_TRY(sort_keys(g, q, n, bits + 1, svo, timer, [&]() { return vrc::launch_edit_keys(q, g->stream); }));
    if (!svo) HIP_TRY(g, vrc::launch_edit_array(q, g->stream));
    HIP_TRY(g, timer.end(c, q.counters, sizeof(c)));
    st.skipped = (int64_t)c[vrc::kEditSkipped];
    if (!svo) { st.changed = (int64_t)c[vrc::kEditChanged]; return VRC_OK; }

    // the touched bricks (the last run is the skipped edits'), and from their keys the touched nodes of every level above them
    const int64_t nb = (int64_t)c[vrc::kEditRuns] - (st.skipped > 0 ? 1 : 0);
    if (nb <= 0) return VRC_OK;
    return edit_append(g, q, nullptr, nb, c, timer, st, "set_voxels");
}

// One handle's region edit up to the commit, as edit_stage: the front end that turns operations into (brick, operation) pairs
// without enumerating a voxel (region_write.hip), then the map's brick pass or the SVO edit's own tail.
int region_stage(vrc_caster *g, const EditBatch &b, const int32_t *d_first, const void *d_second, EditStage &st) {
    vrc::RegionParams rp;
    memset(&rp, 0, sizeof(rp));
    vrc::EditParams &q = rp.edit;
    std::unique_lock<std::mutex> lock;
    SegmentTimer timer;
    VRC_TRY(stage_begin(g, st, lock, timer, q.scene, &q.counters));
    const int64_t n = b.n;
    const bool svo = q.scene.svo != 0;
    const int nlog = q.scene.log2_dim, above = std::max(nlog - vrc::kReadBrickLog2, 0);
    const bool paste = b.kind == kPaste;
    const bool shapes = b.kind == kShapes;
    rp.boxes = d_first; rp.n = n; rp.mode = paste ? vrc::kRegionPaste : shapes ? vrc::kRegionShapes : vrc::kRegionFill; rp.flags = b.flags; rp.volume = b.volume;
    if (paste) rp.data = static_cast<const int8_t *>(d_second); else rp.materials = static_cast<const int32_t *>(d_second);
    for (int a = 0; a < 3; a++) { rp.size[a] = b.size[a]; rp.lim[a] = q.scene.map_dim[a]; }
    // the map's rows at z >= dy have an index past the array (dy <= dz: edit_call): they are outside the scene
    if (!svo) rp.lim[2] = std::min(rp.lim[2], rp.lim[1]);
    for (int a = 0; a < 3; a++) rp.nb[a] = ((int64_t)rp.lim[a] + 7) / 8;
    int bits = 3 * above;
    if (!svo)
        for (bits = 0; bits < 63 && (1ULL << bits) < (uint64_t)(rp.nb[0] * rp.nb[1] * rp.nb[2]); bits++) {}
    bits = std::max(bits, 1);
    const bool have = g->tree->d_attach_lookup && g->tree->d_attach;
    rp.scan_materials = svo && paste && !have;
    q.map = g->d_map;
    VRC_TRY(grow(g, g->region_capacity, n + 1, {{g->d_region_counts, sizeof(uint64_t) * 2 * (size_t)(n + 1)}}));
    rp.counts = g->d_region_counts; rp.offsets = g->d_region_counts + (n + 1);
    size_t scan_bytes = 0;
    HIP_TRY(g, vrc::region_scan(nullptr, &scan_bytes, rp.counts, rp.offsets, n + 1, g->stream));
    scan_bytes = std::max<size_t>(scan_bytes, 16);
    VRC_TRY(grow(g, g->edit_temp_bytes, scan_bytes, {{g->d_edit_temp, scan_bytes}}));
    unsigned long long c[vrc::kEditCounters];
    uint64_t pairs = 0;

    // the bricks every operation overlaps, their scan, and the one read-back the sizes of everything else depend on
    HIP_TRY(g, hipMemsetAsync(q.counters, 0, sizeof(c), g->stream));
    HIP_TRY(g, timer.start());
    HIP_TRY(g, shapes ? vrc::launch_shape_count(rp, g->stream) : vrc::launch_region_count(rp, g->stream));
    if (rp.scan_materials) HIP_TRY(g, vrc::launch_region_materials(rp, g->stream));
    HIP_TRY(g, vrc::region_scan(g->d_edit_temp, &scan_bytes, rp.counts, rp.offsets, n + 1, g->stream));
    HIP_TRY(g, timer.stop());
    HIP_TRY(g, hipMemcpyAsync(c, q.counters, sizeof(c), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(g, hipMemcpyAsync(&pairs, rp.offsets + n, sizeof(pairs), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(g, timer.wait());
    st.skipped = (int64_t)c[vrc::kEditSkipped];
    if (pairs == 0) return VRC_OK;
    if (pairs > (uint64_t)INT32_MAX) return fail(g, VRC_ERR_LIMIT, "%s: more than 2^31 - 1 (brick, operation) pairs", b.what);

    // the pairs, sorted by brick (stable: a brick's operations stay in index order), and the touched bricks in key order
    VRC_TRY(sort_keys(g, q, (int64_t)pairs, bits, true, timer, [&]() { return shapes ? vrc::launch_shape_emit(rp, g->stream) : vrc::launch_region_emit(rp, g->stream); }));
    HIP_TRY(g, timer.end(c + vrc::kEditRuns, q.counters + vrc::kEditRuns, sizeof(c[0])));
    const int64_t nb = (int64_t)c[vrc::kEditRuns];
    if (nb <= 0) return VRC_OK;
    if (svo) return edit_append(g, q, &rp, nb, c, timer, st, b.what);

    // the map: one wave per touched brick of the map, in place
    q.brick_keys = g->d_edit_unique; q.n_bricks = nb;
    HIP_TRY(g, timer.start());
    HIP_TRY(g, vrc::launch_region_bricks(rp, g->stream));
    HIP_TRY(g, timer.end(c, q.counters, sizeof(c)));
    st.changed = (int64_t)c[vrc::kEditChanged];
    return VRC_OK;
}

int edit_run(vrc_caster *h, const EditBatch &b, vrc_edit_info *info) {
    if (info && info->struct_size < sizeof(uint32_t)) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: info->struct_size is not set", b.what);
    vrc_edit_info out;
    memset(&out, 0, sizeof(out));
    const bool svo = setting_or(h, "using_octree", 0) == 0;
    DeviceRestore restore;
    if (b.n > 0) {
        std::vector<std::unique_ptr<EditStage>> stages;
        VRC_TRY(run_group(h, svo, stages, [&](vrc_caster *g, EditStage &st) -> int {
            const void *d_first = b.first, *d_second = b.second;
            if (!b.on_device || g->device != h->device) {             // staged: the host's arrays, or rank 0's for a rank on another GPU
                const size_t second_at = (b.first_bytes() + 15) & ~(size_t)15, bytes = second_at + b.second_bytes();
                VRC_TRY(grow(g, g->region_in_bytes, bytes, {{g->d_region_in, bytes}}));
                HIP_TRY(g, hipMemcpyAsync(g->d_region_in, b.first, b.first_bytes(), hipMemcpyDefault, g->stream));
                HIP_TRY(g, hipMemcpyAsync(static_cast<char *>(g->d_region_in) + second_at, b.second, b.second_bytes(), hipMemcpyDefault, g->stream));
                d_first = g->d_region_in; d_second = static_cast<const char *>(g->d_region_in) + second_at;
            } else {
                VRC_TRY(wait_for_null_stream(g));
            }
            if (b.kind != kPoints) return region_stage(g, b, static_cast<const int32_t *>(d_first), d_second, st);
            return edit_stage(g, static_cast<const int32_t *>(d_first), static_cast<const int32_t *>(d_second), b.n, st);
        }));
        const EditStage &s0 = *stages[0];
        out.skipped = s0.skipped; out.voxels_changed = s0.changed; out.seconds = s0.seconds;
        if (svo && s0.commit) { out.bricks_touched = s0.bricks; out.descriptors_added = s0.added; }
    }
    if (svo) {
        out.n_descriptors = h->tree->n_desc;
        out.root_index = (uint64_t)setting_or(h, "octree_root_index", 0);
    }
    if (info) write_info(info, out);
    return VRC_OK;
}

// the two arrays of a _device call: `aligned` names what must be 4-byte aligned (the second array too, unless it holds bytes),
// `readable` both
int write_device_pointers(vrc_caster *h, const void *d_first, const void *d_second, bool second_aligned, const char *aligned, const char *readable,
                          const char *what) {
    if (((uintptr_t)d_first & 3u) || (second_aligned && ((uintptr_t)d_second & 3u)))
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: %s must be 4-byte aligned", what, aligned);
    DeviceRestore restore;
    HIP_TRY(h, hipSetDevice(h->device));
    if (!query_pointer_ok(h, d_first) || !query_pointer_ok(h, d_second))
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: %s must be memory the GPU of the handle (device %d) can read", what, readable, h->device);
    return VRC_OK;
}

// what the four kinds of call differ in before they run: their flag bits and their words for the arrays and for what a batch holds
const struct { uint32_t known; const char *arrays, *items, *aligned, *readable; } kEditKinds[] = {
    {0, "positions or materials", "edits", "positions and materials", "positions and materials"},
    {VRC_WRITE_WHERE_EMPTY | VRC_WRITE_WHERE_SOLID, "boxes or materials", "operations", "boxes and materials", "the arrays"},
    {VRC_WRITE_WHERE_EMPTY | VRC_WRITE_WHERE_SOLID | VRC_WRITE_SKIP_ZERO, "corners or data", "operations", "the corners", "the arrays"},
    {VRC_WRITE_WHERE_EMPTY | VRC_WRITE_WHERE_SOLID, "shapes or materials", "operations", "shapes and materials", "the arrays"},
};

// One call: the argument checks, then the readiness checks of the ray queries and what the branch needs on top, then what only a
// host call can refuse; nothing is launched when one fails.  size / n_bytes: the pastes' block and bytes of data.
int edit_call(vrc_caster *h, EditBatch b, const int32_t *size, size_t n_bytes, vrc_edit_info *info) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    const auto &k = kEditKinds[b.kind];
    const char *what = b.what;
    if (b.n < 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", what, (long long)b.n);
    if (b.kind == kPaste) {
        size_t total = 0;
        VRC_TRY(size_check(h, size, what));
        VRC_TRY(volume_check(h, b.n, size, n_bytes, "data", &b.volume, &total, what));
        memcpy(b.size, size, sizeof(b.size));
    }
    if (b.flags & ~k.known) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", what, (unsigned)(b.flags & ~k.known));
    if ((b.flags & VRC_WRITE_WHERE_EMPTY) && (b.flags & VRC_WRITE_WHERE_SOLID))
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: WHERE_EMPTY and WHERE_SOLID exclude each other", what);
    if (b.n > 0 && (!b.first || !b.second)) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: null %s", what, k.arrays);
    if (b.n > INT32_MAX) return fail(h, VRC_ERR_LIMIT, "%s: more than 2^31 - 1 %s in one batch", what, k.items);
    VRC_TRY(query_check(h, b.first, b.n, 0, 0, b.second, what));
    if (setting_or(h, "using_octree", 0) == 0) {
        VRC_TRY(group_alone_holds_trees(h, what));
    } else if (b.kind != kPoints) {
        // the region edits on the array branch: with dy > dz the frame's index x + dx * (y + dz * z) is not one-to-one over map_dim
        if (h->map_dim[1] > h->map_dim[2]) return fail(h, VRC_ERR_LIMIT, "%s: a map with dy = %d > dz = %d has voxels that share a byte", what, h->map_dim[1], h->map_dim[2]);
        for (const vrc_caster *g : h->peers)
            if (g->map_dim[1] > g->map_dim[2]) return fail(h, VRC_ERR_LIMIT, "%s: a rank's map has dy > dz", what);
    }
    if (b.n > 0 && b.on_device) VRC_TRY(write_device_pointers(h, b.first, b.second, b.kind != kPaste, k.aligned, k.readable, what));
    const int32_t *boxes = static_cast<const int32_t *>(b.first), *materials = static_cast<const int32_t *>(b.second);
    for (int64_t i = 0; i < b.n && !b.on_device && b.kind != kPaste; i++) {
        if (materials[i] < -128 || materials[i] > 127)
            return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: materials[%lld] = %d is outside [-128, 127]", what, (long long)i, (int)materials[i]);
        for (int a = 0; a < 3 && b.kind == kFill; a++)
            if (boxes[6 * i + 3 + a] < 1)
                return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: box %lld has size[%d] = %d < 1", what, (long long)i, a, (int)boxes[6 * i + 3 + a]);
        if (b.kind == kShapes) {
            const int32_t *s = boxes + 6 * i;
            if (!vrc::shape_valid(vrc::ShapeOp{s[0], {s[1], s[2], s[3]}, s[4], s[5]}, materials[i]))
                return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: shape %lld has kind = %d, r = %d, h = %d: the kind is 0 .. 3, r is in [0, 2^30], a ball has h = 0 and a cylinder h >= 1",
                            what, (long long)i, (int)s[0], (int)s[4], (int)s[5]);
        }
    }
    return edit_run(h, b, info);
}

// ---------------------------------------------------------------------------------------------------------------------------
// octree compaction (vrc_compact_octree, octree_compact.hip)
// ---------------------------------------------------------------------------------------------------------------------------

// device memory of one call: the lists, scans and sizes of every level.  Freed when the call ends, so none of it outlives the tree.
struct CompactScratch {
    int device = 0;
    std::vector<void *> held;
    explicit CompactScratch(int dev) : device(dev) {}
    CompactScratch(const CompactScratch &) = delete;
    CompactScratch &operator=(const CompactScratch &) = delete;
    template <class T>
    hipError_t get(T *&p, uint64_t n) {
        void *v = nullptr;
        const hipError_t e = hipMalloc(&v, (size_t)std::max<uint64_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) { held.push_back(v); p = static_cast<T *>(v); }
        return e;
    }
    ~CompactScratch() {
        DeviceRestore restore;
        (void)hipSetDevice(device);
        for (void *v : held) (void)hipFree(v);
        (void)hipGetLastError();
    }
};

// What one handle's compaction has prepared: the staged arrays edit_commit installs, and the counts of vrc_compact_info.
struct CompactStage : EditStage {
    uint64_t before = 0, far = 0, attach_before = 0;
};

// One handle's compaction up to the commit (current device: g->device).  dry: sweeps 1 and 2 and the used attachment slots only.
int compact_stage(vrc_caster *g, bool dry, CompactStage &st) {
    const char *what = "compact_octree";
    vrc::CompactParams q;
    memset(&q, 0, sizeof(q));
    std::unique_lock<std::mutex> lock;
    SegmentTimer timer;                  // (the kernels run in segments, each ended by the read-back that sizes the next one)
    VRC_TRY(stage_begin(g, st, lock, timer, q.scene));
    vrc_tree *t = g->tree.get();
    const int n = q.scene.log2_dim;
    const bool have = q.scene.attach_lookup != nullptr;
    q.n_old = t->n_desc;
    q.n_attach_old = have ? std::max<uint64_t>(t->n_attach, 1) : 0;
    q.reach = (uint64_t)setting_or(g, "compact_near_reach", vrc::kCompactReachMax);
    st.before = q.n_old; st.attach_before = q.n_attach_old;
    CompactScratch mem(g->device);
    auto scan = [&](const uint64_t *in, uint64_t *out, uint64_t count) {
        size_t bytes = 0;
        char *temp = nullptr;
        hipError_t e = vrc::compact_scan(nullptr, &bytes, in, out, count, g->stream);
        if (e == hipSuccess) e = mem.get(temp, bytes);
        if (e == hipSuccess) e = vrc::compact_scan(temp, &bytes, in, out, count, g->stream);
        return e;
    };
    HIP_TRY(g, mem.get(q.counters, vrc::kCompactCounters));
    HIP_TRY(g, hipMemsetAsync(q.counters, 0, sizeof(unsigned long long) * vrc::kCompactCounters, g->stream));

    // sweep 1, top-down: the pointer-holding descriptors of every level above the bottom
    uint64_t root_word = 0;
    HIP_TRY(g, hipMemcpy(&root_word, t->d_desc + q.scene.root_index, sizeof(root_word), hipMemcpyDeviceToHost));
    std::vector<vrc::CompactLevel> levels;
    uint64_t count = (n > 1 && ((root_word >> 16) & 0xffULL)) ? 1 : 0;
    uint64_t *list = nullptr;
    if (count) {
        HIP_TRY(g, mem.get(list, 1));
        HIP_TRY(g, hipMemcpy(list, &q.scene.root_index, sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    for (int l = 0; l <= n - 2 && count > 0; l++) {
        vrc::CompactLevel L;
        memset(&L, 0, sizeof(L));
        L.list = list; L.count = (int64_t)count; L.level = l; L.children_bottom = l == n - 2 ? 1 : 0;
        uint64_t *sums = nullptr, *base = nullptr;
        HIP_TRY(g, mem.get(L.pmask, count)); HIP_TRY(g, mem.get(L.farmask, count)); HIP_TRY(g, mem.get(L.size, count));
        HIP_TRY(g, mem.get(L.cnt, count + 1)); HIP_TRY(g, mem.get(sums, count + 1)); HIP_TRY(g, mem.get(base, count));
        L.scan = sums; L.base = base;
        HIP_TRY(g, timer.start());
        if (!levels.empty()) HIP_TRY(g, vrc::launch_compact_level(q, levels.back(), 1, g->stream));    // (this level's list)
        HIP_TRY(g, vrc::launch_compact_level(q, L, 0, g->stream));
        HIP_TRY(g, scan(L.cnt, sums, count + 1));
        HIP_TRY(g, timer.end());
        uint64_t next = 0;
        HIP_TRY(g, hipMemcpy(&next, sums + count, sizeof(next), hipMemcpyDeviceToHost));
        if (next > q.n_old) return fail(g, VRC_ERR_INVALID_ARGUMENT, "%s: level %d holds more descriptors than the array: not a tree", what, l + 1);
        list = nullptr;
        if (next) HIP_TRY(g, mem.get(list, next));
        L.next_list = list;
        levels.push_back(L);
        count = next;
    }
    if (count) return fail(g, VRC_ERR_INVALID_ARGUMENT, "%s: the bottom level holds pointers: not a tree", what);
    for (size_t l = 0; l + 1 < levels.size(); l++) { levels[l].size_below = levels[l + 1].size; levels[l].base_below = const_cast<uint64_t *>(levels[l + 1].base); }

    // sweep 2, bottom-up: the subtree sizes and the far children
    uint64_t below_root = 0;
    if (!levels.empty()) {
        HIP_TRY(g, timer.start());
        for (size_t l = levels.size(); l-- > 0;) HIP_TRY(g, vrc::launch_compact_level(q, levels[l], 2, g->stream));
        HIP_TRY(g, timer.end());
        HIP_TRY(g, hipMemcpy(&below_root, levels[0].size, sizeof(below_root), hipMemcpyDeviceToHost));
    }
    unsigned long long c[vrc::kCompactCounters];
    HIP_TRY(g, hipMemcpy(c, q.counters, sizeof(c), hipMemcpyDeviceToHost));
    if (c[vrc::kCompactBad]) return fail(g, VRC_ERR_INVALID_ARGUMENT, "%s: the tree points outside its array (%llu indices)", what, c[vrc::kCompactBad]);
    st.n_desc = 1 + below_root; st.far = c[vrc::kCompactFar]; st.root = 0;
    if (st.n_desc >= (1ULL << 47)) return fail(g, VRC_ERR_LIMIT, "%s: more than 2^47 descriptors", what);

    // the new arrays, beside the old ones until the commit
    const size_t free_b = free_device_bytes();
    if (!dry) {
        VRC_TRY(stage_array(g, st.desc, st.cap_desc, st.n_desc, free_b, what));
        q.out = st.desc; q.n_out = st.n_desc;
        if (have) {
            VRC_TRY(stage_array(g, st.lookup, st.cap_lookup, st.n_desc, free_b, what));
            HIP_TRY(g, hipMemsetAsync(st.lookup, 0, st.n_desc * sizeof(uint32_t), g->stream));
            q.out_lookup = st.lookup;
        }
        if (!levels.empty()) {
            const uint64_t one = 1;
            HIP_TRY(g, hipMemcpy(const_cast<uint64_t *>(levels[0].base), &one, sizeof(one), hipMemcpyHostToDevice));
        }
    }
    uint64_t *remap = nullptr;
    if (have) {
        HIP_TRY(g, mem.get(q.used, q.n_attach_old + 1));
        HIP_TRY(g, mem.get(remap, q.n_attach_old + 1));
        HIP_TRY(g, hipMemsetAsync(q.used, 0, (q.n_attach_old + 1) * sizeof(uint64_t), g->stream));
    }

    // sweep 3, top-down: the blocks, the far slots, the lookup words, the used attachment slots (a dry run: only those, which
    // the parents of the bottom level raise)
    HIP_TRY(g, timer.start());
    if (!dry || have) HIP_TRY(g, vrc::launch_compact_root(q, g->stream));
    for (const vrc::CompactLevel &L : levels)
        if (!dry || (have && L.children_bottom)) HIP_TRY(g, vrc::launch_compact_level(q, L, 3, g->stream));
    if (have) HIP_TRY(g, scan(q.used, remap, q.n_attach_old + 1));
    HIP_TRY(g, timer.end());
    if (have) {
        uint64_t kept = 0;
        HIP_TRY(g, hipMemcpy(&kept, remap + q.n_attach_old, sizeof(kept), hipMemcpyDeviceToHost));
        st.n_attach = std::max<uint64_t>(kept, 1);                   // (a tree with materials keeps a slot: slot 0 = eight 5s, as the edit creates it)
        if (!dry) {
            VRC_TRY(stage_array(g, st.attach, st.cap_attach, st.n_attach, free_b, what));
            HIP_TRY(g, timer.start());
            if (!kept) HIP_TRY(g, hipMemsetAsync(st.attach, 0x05, sizeof(uint64_t), g->stream));
            HIP_TRY(g, vrc::launch_compact_materials(q, remap, st.n_desc, st.attach, kept, g->stream));
            HIP_TRY(g, timer.end());
        }
    }
    HIP_TRY(g, hipMemcpy(c, q.counters, sizeof(c), hipMemcpyDeviceToHost));
    if (c[vrc::kCompactBad]) return fail(g, VRC_ERR_INVALID_ARGUMENT, "%s: the tree points outside its array (%llu indices)", what, c[vrc::kCompactBad]);
    st.commit = !dry;
    return VRC_OK;
}

int compact_run(vrc_caster *h, bool dry, vrc_compact_info *info) {
    vrc_compact_info out;
    memset(&out, 0, sizeof(out));
    DeviceRestore restore;
    if (setting_or(h, "using_octree", 0) == 0) {
        std::vector<std::unique_ptr<CompactStage>> stages;
        VRC_TRY(run_group(h, true, stages, [&](vrc_caster *g, CompactStage &st) { return compact_stage(g, dry, st); }));
#ifdef VRC_INDEX_AUDIT
        // the tables still hold the old tree's extents, and the new arrays are SHORTER: what runs next is held against the new ones
        for (vrc_caster *g : dry ? std::vector<vrc_caster *>() : group_of(h)) {
            HIP_TRY(h, hipSetDevice(g->device));
            std::lock_guard<std::mutex> lock(g->tree->guard);
            AuditExtents x;
            audit_tree(x, g->tree.get());
            VRC_AUDIT_PUBLISH(h, x);
        }
        HIP_TRY(h, hipSetDevice(h->device));
#endif
        const CompactStage &s0 = *stages[0];
        out.descriptors_before = s0.before; out.n_descriptors = s0.n_desc; out.root_index = 0;
        out.live_descriptors = s0.n_desc - s0.far; out.far_slots = s0.far;
        out.attachments_before = s0.attach_before; out.n_attachments = s0.n_attach;
        out.seconds = s0.seconds;
    }
    if (info) write_info(info, out);
    return VRC_OK;
}

}  // namespace

extern "C" {

int vrc_set_voxels(vrc_caster *h, const int32_t *positions, const int32_t *materials, int64_t n, uint32_t flags, vrc_edit_info *info) {
    return edit_call(h, {"set_voxels", positions, materials, n, false, kPoints, flags}, nullptr, 0, info);
}
int vrc_set_voxels_device(vrc_caster *h, const void *d_positions, const void *d_materials, int64_t n, uint32_t flags, vrc_edit_info *info) {
    return edit_call(h, {"set_voxels_device", d_positions, d_materials, n, true, kPoints, flags}, nullptr, 0, info);
}
int vrc_fill_boxes(vrc_caster *h, const int32_t *boxes, const int32_t *materials, int64_t n, uint32_t flags, vrc_edit_info *info) {
    return edit_call(h, {"fill_boxes", boxes, materials, n, false, kFill, flags}, nullptr, 0, info);
}
int vrc_fill_boxes_device(vrc_caster *h, const void *d_boxes, const void *d_materials, int64_t n, uint32_t flags, vrc_edit_info *info) {
    return edit_call(h, {"fill_boxes_device", d_boxes, d_materials, n, true, kFill, flags}, nullptr, 0, info);
}
int vrc_fill_shapes(vrc_caster *h, const int32_t *shapes, const int32_t *materials, int64_t n, uint32_t flags, vrc_edit_info *info) {
    return edit_call(h, {"fill_shapes", shapes, materials, n, false, kShapes, flags}, nullptr, 0, info);
}
int vrc_fill_shapes_device(vrc_caster *h, const void *d_shapes, const void *d_materials, int64_t n, uint32_t flags, vrc_edit_info *info) {
    return edit_call(h, {"fill_shapes_device", d_shapes, d_materials, n, true, kShapes, flags}, nullptr, 0, info);
}
int vrc_write_regions(vrc_caster *h, const int32_t *lo, int64_t n, const int32_t size[3], const int8_t *data, size_t n_bytes, uint32_t flags, vrc_edit_info *info) {
    return edit_call(h, {"write_regions", lo, data, n, false, kPaste, flags}, size, n_bytes, info);
}
int vrc_write_regions_device(vrc_caster *h, const void *d_lo, int64_t n, const int32_t size[3], const void *d_data, size_t n_bytes, uint32_t flags, vrc_edit_info *info) {
    return edit_call(h, {"write_regions_device", d_lo, d_data, n, true, kPaste, flags}, size, n_bytes, info);
}

int vrc_compact_octree(vrc_caster *h, uint32_t flags, vrc_compact_info *info) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    const char *what = "compact_octree";
    if (flags & ~(uint32_t)VRC_COMPACT_DRY_RUN) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", what, (unsigned)(flags & ~(uint32_t)VRC_COMPACT_DRY_RUN));
    if (info && info->struct_size < sizeof(uint32_t)) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: info->struct_size is not set", what);
    const int64_t reach = setting_or(h, "compact_near_reach", vrc::kCompactReachMax);
    if (reach < vrc::kCompactReachMin || reach > vrc::kCompactReachMax)
        return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: compact_near_reach = %lld is outside [%lld, %lld]", what, (long long)reach, (long long)vrc::kCompactReachMin, (long long)vrc::kCompactReachMax);
    VRC_TRY(query_check(h, nullptr, 0, 0, 0, nullptr, what));
    if (setting_or(h, "using_octree", 0) == 0) VRC_TRY(group_alone_holds_trees(h, what));
    return compact_run(h, (flags & VRC_COMPACT_DRY_RUN) != 0, info);
}

}  // extern "C"
