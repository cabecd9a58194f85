// The device walkers' shared code (csrc/svo_node.hpp) on the host, under AddressSanitizer + UBSan: the region descent and the
// point form against dense material grids.  Built and run by tests/test_svo_node_cpu.py.
//
// usage: svo_node_check <tree file> <grid file> [<tree file> <grid file> ...]
//   tree file: vrc_octree_save's, with attachments; grid file: dim^3 int8 materials, index x + dim * (y + dim * z)
// Every tree is walked from the root and, where it is deep enough for one, from coarse tables (built here the way
// coarse_build_kernel builds them) of the coarsest and the finest level the host layer would take.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svo_node.hpp"
#include "vrc.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "check failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

using namespace vrc;

// the table of 2^lc cells per axis: the cursor state of the descent toward each cell
static std::vector<uint64_t> coarse_table(const SceneView &s, int lc) {
    const int n = s.log2_dim, sh = n - lc;
    std::vector<uint64_t> out((size_t)1 << (3 * lc));
    for (unsigned cz = 0; cz < 1u << lc; cz++)
        for (unsigned cy = 0; cy < 1u << lc; cy++)
            for (unsigned cx = 0; cx < 1u << lc; cx++) {
                uint64_t cur = node_entry(s.descriptors, s.root_index, s.descriptors[s.root_index]);
                int top = 0;
                while (top < lc) {
                    const int i = child_slot((int)(cx << sh), (int)(cy << sh), (int)(cz << sh), n - top - 1);
                    const unsigned masks = (unsigned)cur & 0xffffu, bit = 1u << i;
                    if (!(masks & bit) || ((masks >> 8) & bit)) break;
                    const uint64_t child = kept_child(cur, (unsigned)i);
                    cur = node_entry(s.descriptors, child, s.descriptors[child]);
                    top++;
                }
                out[coarse_index(cx, cy, cz, lc)] = coarse_cell_pack(cur, top);
            }
    return out;
}

int main(int argc, char **argv) {
    long far_pointers = 0, table_starts = 0, moved_roots = 0;
    CHECK(argc >= 3 && argc % 2 == 1);
    for (int t = 1; t < argc; t += 2) {
        uint32_t dim = 0, *lookup = nullptr;
        uint64_t *desc = nullptr, n_desc = 0, root = 0, *att = nullptr, n_att = 0;
        CHECK(vrc_octree_load(argv[t], &dim, &desc, &n_desc, &root, &lookup, &att, &n_att) == VRC_OK);
        CHECK(lookup && att);
        std::vector<int8_t> grid((size_t)dim * dim * dim);
        FILE *f = fopen(argv[t + 1], "rb");
        CHECK(f && fread(grid.data(), 1, grid.size(), f) == grid.size());
        fclose(f);
        int n = 0;
        while ((1u << n) < dim) n++;
        SceneView s = {};
        s.svo = 1;
        s.map_dim[0] = s.map_dim[1] = s.map_dim[2] = (int32_t)dim;
        s.descriptors = desc; s.root_index = root; s.log2_dim = n;
        s.attach_lookup = lookup; s.attachments = att;
        moved_roots += root != 0;
        std::vector<int> levels = {0};                     // 0: no table; a table has 1 <= lc <= n - 2
        if (n - 2 >= 1) levels.push_back(1);
        if (n - 2 > 1) levels.push_back(n - 2);
        for (int lc : levels) {
            std::vector<uint64_t> table;
            if (lc >= 1) { table = coarse_table(s, lc); s.coarse = table.data(); s.coarse_log2 = lc; }
            else { s.coarse = nullptr; s.coarse_log2 = 0; }
            for (int r = 0; r <= n; r++) {
                const int size = 1 << r;
                for (int z = 0; z < (int)dim; z += size)
                    for (int y = 0; y < (int)dim; y += size)
                        for (int x = 0; x < (int)dim; x += size) {
                            uint64_t cur = 0, index = 0;
                            const int state = descend_to_node(s, x, y, z, r, cur, index);
                            CHECK(state >= 0 && state <= 3 && (state != 3 || r == 0) && (state != 2 || r >= 1));
                            if (s.coarse && r <= n - lc) table_starts++;
                            if (state == 2) {
                                // a node below the root that is a table cell's own comes without its index; every other index is the
                                // descriptor the entry was made from (the header against itself: the grids are the independent reference)
                                if (s.coarse && r == n - lc && r < n) CHECK(index == kNoIndex);
                                else CHECK(index < n_desc && cur == node_entry(desc, index, desc[index]));
                                // far-flagged descriptors the descent arrived at, each once: their entry `cur` came through the far slot
                                if (lc == 0 && r >= 2 && (desc[index] & kFarBit) && (desc[index] & kValidAll)) far_pointers++;
                                continue;
                            }
                            for (int dz = 0; dz < size; dz++)
                                for (int dy = 0; dy < size; dy++)
                                    for (int dx = 0; dx < size; dx++) {
                                        const int8_t m = grid[(size_t)(x + dx) + dim * ((size_t)(y + dy) + (size_t)dim * (z + dz))];
                                        CHECK(state == 0 ? m == 0 : m != 0);
                                    }
                        }
            }
            for (int z = 0; z < (int)dim; z++)
                for (int y = 0; y < (int)dim; y++)
                    for (int x = 0; x < (int)dim; x++)
                        CHECK(voxel_material(s, x, y, z) == (int)grid[(size_t)x + dim * ((size_t)y + (size_t)dim * z)]);
        }
        // ... and the reference's descent finds what the point form finds
        for (int z = 0; z < (int)dim; z++)
            for (int y = 0; y < (int)dim; y++)
                for (int x = 0; x < (int)dim; x++) {
                    const int pos[3] = {x, y, z};
                    const OctVox v = get_oct_vox(desc, root, (int)dim, pos);
                    CHECK((v.found != 0) == (grid[(size_t)x + dim * ((size_t)y + (size_t)dim * z)] != 0));
                    CHECK(v.reads >= 1 && v.reads <= (n > 1 ? n : 1));
                    for (int a = 0; a < 3; a++) CHECK(v.corner[a] <= pos[a]);
                }
        vrc_free(desc); vrc_free(lookup); vrc_free(att);
    }
    printf("svo node ok: trees %d, far pointers %ld, table starts %ld, moved roots %ld\n", (argc - 1) / 2, far_pointers, table_starts, moved_roots);
    return 0;
}
