"""A hand-made descriptor array with solid leaves above the bottom level (the leaf bit of a valid slot: a solid cube of the
slot's size), built like treetools.sparse_octree: root first, every node's valid children in one block in slot order
(i = x | y<<1 | z<<2), blocks in breadth-first order, near pointers only.  A leaf slot keeps its place in the block (the child
rank counts every valid slot) but its descriptor is never read.  Not a test file."""
import numpy as np


def leaf_octree(voxels, cubes, depth):
    """voxels: solid voxels at the bottom level; cubes: (x, y, z, size) aligned solid leaves, size a power of two in
    [2, 2^(depth-1)].  Returns (descriptors, root_index, dense int8 grid, index x + dim * (y + dim * z), solid = 5)."""
    dim = 1 << depth
    leaves = {(int(x), int(y), int(z), int(s)) for x, y, z, s in cubes}
    vox = sorted({tuple(int(c) for c in v) for v in voxels})

    def build(ox, oy, oz, size, vs):
        half = size // 2
        if size == 2:
            return sum(1 << ((x - ox) | ((y - oy) << 1) | ((z - oz) << 2)) for x, y, z in vs)
        node = {}
        for i in range(8):
            cx, cy, cz = ox + (i & 1) * half, oy + ((i >> 1) & 1) * half, oz + ((i >> 2) & 1) * half
            if (cx, cy, cz, half) in leaves:
                node[i] = "LEAF"
                continue
            sub = [v for v in vs if cx <= v[0] < cx + half and cy <= v[1] < cy + half and cz <= v[2] < cz + half]
            inner = any(cx <= x < cx + half and cy <= y < cy + half and cz <= z < cz + half and s < half for x, y, z, s in leaves)
            if sub or inner:
                node[i] = build(cx, cy, cz, half, sub)
        return node

    root = build(0, 0, 0, dim, vox)
    out, queue = [0], [(0, root, dim)]
    while queue:
        index, node, size = queue.pop(0)
        if size == 2:
            out[index] = (node << 16) | (0xff << 24)
            continue
        valid = sum(1 << i for i in node)
        leaf = sum(1 << i for i, c in node.items() if c == "LEAF")
        first = len(out)
        assert first - index < 0x8000, "leaf_octree: near pointers only"
        for i in sorted(node):
            if node[i] != "LEAF":
                queue.append((len(out), node[i], size // 2))
            out.append(0)
        out[index] = (first - index) | (valid << 16) | (leaf << 24)
    grid = np.zeros((dim, dim, dim), np.int8)                  # [z, y, x]
    for x, y, z in vox:
        grid[z, y, x] = 5
    for x, y, z, s in leaves:
        grid[z:z + s, y:y + s, x:x + s] = 5
    return np.array(out, dtype=np.uint64), 0, grid.reshape(-1)
