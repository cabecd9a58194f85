"""Test helper: the same octree in another array.  relayout() moves the root and every block of children of a descriptor array
(format of include/map/Octree.h:89-94) to random places -- child blocks before their parents, far pointers, a root in the
middle of the array, unreferenced words between the blocks -- and decode() reads any such array back into a dense grid on the
host.  The small, exhaustively compared trees of the suite are breadth-first with near pointers only; through relayout() they
reach every tree-walking kernel with the features only the large device-built terrains had.  Not a test file."""
import numpy as np

import leaftree

FAR = 0x8000
# every slot valid and leaf, offset 0: a kernel that wrongly reads a filler word sees solid matter and follows no pointer
FILLER = 0xFFFF0000


def _walk(d, root, dim):
    """Units (first old index, words) -- the root, then every block of valid children in the order a walk from the root meets
    them --, the parents [(old index, unit of its block)], and the reachable old indices with the size of their node."""
    units, parents, reach = [(int(root), 1)], [], {}
    stack = [(int(root), int(dim))]
    while stack:
        index, size = stack.pop()
        assert index not in reach, "relayout: a descriptor reached twice"
        reach[index] = size
        if size == 2:
            continue
        v = d[index]
        valid, leaf = (v >> 16) & 0xff, (v >> 24) & 0xff
        if not valid:
            continue
        at = index + (v & 0x7fff)
        if v & FAR:
            at = d[at]
        parents.append((index, len(units)))
        units.append((at, bin(valid).count("1")))
        k = 0
        for i in range(8):
            if valid >> i & 1:
                if not (leaf >> i & 1):                       # a leaf slot keeps its place; its descriptor is never read
                    stack.append((at + k, size // 2))
                k += 1
    return units, parents, reach


def relayout(desc, root, dim, rng, far_fraction, lookup=None, filler=FILLER):
    """(desc2, root2, lookup2): the tree of (desc, root) with the root and every child block placed as units in a random order,
    0 to 2 filler words between units (at least one before a root that comes first: index 0 is never the root), the far slots of
    a unit's descriptors right behind it.  A parent whose block lies behind it or 0x8000 or more ahead gets a far pointer (bit 15
    + the offset of a slot holding the absolute index), and so does a far_fraction share of the others.  Masks, bottom-level
    words and leaf slots are carried over unchanged; lookup2[new] = lookup[old] for every reachable descriptor, 0 elsewhere."""
    d = [int(v) for v in np.asarray(desc).reshape(-1)]
    units, parents, reach = _walk(d, root, dim)
    order = [int(u) for u in rng.permutation(len(units))]
    gaps = [int(g) for g in rng.integers(0, 3, size=len(units) + 1)]
    if order[0] == 0 and gaps[0] == 0:
        gaps[0] = 1
    wants_far = {p: bool(rng.random() < far_fraction) for p, _ in parents}
    block_of = dict(parents)
    unit_of = {}                                              # old index -> (unit, offset in it)
    for u, (first, n) in enumerate(units):
        for k in range(n):
            assert first + k not in unit_of, "relayout: two blocks share a word"
            unit_of[first + k] = (u, k)
    far = {p for p, w in wants_far.items() if w}
    while True:                                               # a far slot moves what follows: repeat until no pointer is out of reach
        start, slot, at = {}, {}, 0
        for j, u in enumerate(order):
            at += gaps[j]
            start[u] = at
            first, n = units[u]
            at += n
            for k in range(n):
                if first + k in far:
                    slot[first + k] = at
                    at += 1
        total = at + gaps[-1]
        new = {old: start[u] + k for old, (u, k) in unit_of.items()}
        more = {p for p, b in parents if p not in far and not (0 < start[b] - new[p] < 0x8000)}
        if not more:
            break
        far |= more
    out = [int(filler)] * total
    for old, (u, k) in unit_of.items():
        v = d[old]
        if old in block_of and old in reach:
            v &= ~0xffff
            if old in far:
                assert 0 <= slot[old] - new[old] < 0x8000
                v |= FAR | (slot[old] - new[old])
                out[slot[old]] = start[block_of[old]]
            else:
                assert 0 < start[block_of[old]] - new[old] < 0x8000
                v |= start[block_of[old]] - new[old]
        out[new[old]] = v
    lookup2 = None
    if lookup is not None:
        lookup2 = np.zeros(total, dtype=np.uint32)
        for old in reach:
            lookup2[new[old]] = lookup[old]
    return np.array(out, dtype=np.uint64), new[int(root)], lookup2


def parents_with_children(desc, root, dim):
    """How many descriptors above the bottom level the root reaches that have a valid child: those that hold a pointer."""
    return len(_walk([int(v) for v in np.asarray(desc).reshape(-1)], root, dim)[1])


def decode(desc, root, dim, lookup=None, attachments=None, ignore_far=False):
    """The dense int8 grid (flat, index x + dim * (y + dim * z)) an array encodes from `root`: the attachment byte of a
    bottom-level voxel where lookup / attachments are given, 5 otherwise and for a solid leaf above the bottom.  ignore_far: the
    decoder of a kernel that forgot the far bit (base = index + offset whatever bit 15 says).  An index outside the array raises
    IndexError: the array does not decode."""
    d = [int(v) for v in np.asarray(desc).reshape(-1)]
    grid = np.zeros((dim, dim, dim), dtype=np.int8)           # [z, y, x]

    def at(i):
        if not 0 <= i < len(d):
            raise IndexError(i)
        return d[i]

    def node(index, x, y, z, size):
        v = at(index)
        valid, leaf = (v >> 16) & 0xff, (v >> 24) & 0xff
        half = size // 2
        if size == 2:
            mats = int(attachments[int(lookup[index])]) if lookup is not None else 0x0505050505050505
            for k in range(8):
                if valid >> k & 1:
                    grid[z + (k >> 2 & 1), y + (k >> 1 & 1), x + (k & 1)] = np.uint8(mats >> (8 * k) & 0xff).astype(np.int8)
            return
        base = index + (v & 0x7fff)
        if v & FAR and not ignore_far:
            base = at(base)
        rank = 0
        for k in range(8):
            if not (valid >> k & 1):
                continue
            cx, cy, cz = x + (half if k & 1 else 0), y + (half if k & 2 else 0), z + (half if k & 4 else 0)
            if leaf >> k & 1:
                grid[cz:cz + half, cy:cy + half, cx:cx + half] = 5
            else:
                node(base + rank, cx, cy, cz, half)
            rank += 1

    node(int(root), 0, 0, 0, int(dim))
    return grid.reshape(-1)


def with_materials(grid, seed):
    """The grid with a tenth of its solid voxels rewritten to 6 and a few to -3 (the sign must survive)."""
    g = np.asarray(grid, np.int8).copy().reshape(-1)
    rng = np.random.default_rng(seed)
    solid = np.nonzero(g)[0]
    if solid.size:
        g[rng.choice(solid, size=max(1, solid.size // 10), replace=False)] = 6
        g[rng.choice(solid, size=max(1, solid.size // 50), replace=False)] = -3
    return g


LEAF_CUBES = [(0, 0, 0, 4), (8, 8, 8, 8), (4, 0, 0, 2), (16, 16, 0, 4), (20, 4, 6, 2)]


def leaf_tree(depth=5):
    """leaftree.leaf_octree (solid leaves above the bottom level) with materials on the voxels outside its solid cubes -- a
    solid leaf above the bottom is material 5.  Through relayout() one tree has both solid leaves and far pointers.
    Returns (descriptors, root_index, material grid)."""
    dim = 1 << depth
    rng = np.random.default_rng(5)
    desc, root, grid = leaftree.leaf_octree(rng.integers(0, dim, size=(300, 3)), LEAF_CUBES, depth)
    g = with_materials(grid, 55).reshape(dim, dim, dim)
    for x, y, z, k in LEAF_CUBES:
        g[z:z + k, y:y + k, x:x + k] = 5
    return desc, root, g.reshape(-1)
