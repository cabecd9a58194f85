"""numpy restatement of the octree compaction (vrc_compact_octree, include/vrc.h): what the root reaches, copied into a dense
pre-order array -- the root at 0, then per pointer-holding descriptor its child block (the children, the far slots of its far
children) followed by the children's own blocks in child order.  Bits 16-63 of every copied word are the old word's, bits 0-15
the new pointer (0 where no walker follows one); a child is far when 16 + the subtree words of the children before it exceed
`reach`.  The used attachment slots keep their order.  The test oracle of tests/test_compaction_*.py.  Not a test file."""
import numpy as np

DEFAULT_REACH = 0x7fff
FAR = 0x8000
SOLID = 0x0505050505050505


def compact(desc, root, dim, reach=DEFAULT_REACH, lookup=None, attachments=None):
    """{descriptors, lookup, attachments, info}: the compacted arrays of the tree of (desc, root) -- lookup / attachments None for a
    tree without materials -- and the counts vrc_compact_info reports."""
    d = [int(v) for v in np.asarray(desc).reshape(-1)]
    n = int(dim).bit_length() - 1
    assert 1 << n == dim and n >= 1 and 16 <= reach <= DEFAULT_REACH
    info = {}                                                 # old index of a pointer-holding descriptor -> (children, far slots, S)

    def valid_of(i):
        return d[i] >> 16 & 0xff

    def measure(i, level):
        assert i not in info, "compact: a descriptor reached twice"
        v = d[i]
        valid, leaf = v >> 16 & 0xff, v >> 24 & 0xff
        first = i + (v & 0x7fff)
        if v & FAR:
            first = d[first]
        kids, below, far = [], 0, 0
        for k in range(8):
            if not valid >> k & 1:
                continue
            c = first + len(kids)
            is_leaf = bool(leaf >> k & 1)
            holds = not is_leaf and level + 1 < n - 1 and valid_of(c) != 0
            is_far = holds and 16 + below > reach
            size = measure(c, level + 1) if holds else 0
            kids.append((c, is_leaf, holds, is_far, size))
            far += is_far
            below += size
        info[i] = (kids, far, len(kids) + far + below)
        return info[i][2]

    root = int(root)
    root_holds = n > 1 and valid_of(root) != 0
    total = 1 + (measure(root, 0) if root_holds else 0)
    out = [None] * total
    bottom = []                                               # (new index, old index) of the bottom-level descriptors
    out[0] = (d[root] & ~0xffff) | (1 if root_holds else 0)
    if n == 1:
        bottom.append((0, root))

    def emit(i, level, base):
        kids, far, _ = info[i]
        slot = base + len(kids)
        target = slot + far
        for k, (c, is_leaf, holds, is_far, size) in enumerate(kids):
            w = d[c] & ~0xffff
            if holds:
                if is_far:
                    assert out[slot] is None
                    out[slot] = target
                    w |= FAR | (slot - (base + k))
                    slot += 1
                else:
                    assert 0 < target - (base + k) <= reach
                    w |= target - (base + k)
            assert out[base + k] is None
            out[base + k] = w
            if level + 1 == n - 1 and not is_leaf:
                bottom.append((base + k, c))
            if holds:
                emit(c, level + 1, target)
            target += size

    if root_holds:
        emit(root, 0, 1)
    assert all(w is not None for w in out), "compact: a word of the output is unaccounted for"
    far_slots = sum(f for _, f, _ in info.values())
    res = {"descriptors": np.array(out, dtype=np.uint64), "lookup": None, "attachments": None}
    n_before = n_after = 0
    if lookup is not None:
        a = np.asarray(attachments, dtype=np.uint64).reshape(-1)
        n_before = len(a)
        used = sorted({int(lookup[old]) for _, old in bottom})
        remap = {s: j for j, s in enumerate(used)}
        lk = np.zeros(total, dtype=np.uint32)
        for new, old in bottom:
            lk[new] = remap[int(lookup[old])]
        res["lookup"] = lk
        # (a tree with materials keeps one slot when nothing names any: slot 0 = eight 5s, as the edit creates it)
        res["attachments"] = a[used] if used else np.array([SOLID], dtype=np.uint64)
        n_after = len(res["attachments"])
    res["info"] = {"descriptors_before": len(d), "n_descriptors": total, "root_index": 0, "live_descriptors": total - far_slots,
                   "far_slots": far_slots, "attachments_before": n_before, "n_attachments": n_after}
    return res
