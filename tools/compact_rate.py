"""Compaction rate (vrc_compact_octree, csrc/octree_compact.hip) on the depth-12 device-built bench scene -- a tree that exists
only in HBM.  The three batches of tools/edit_rate.py (one voxel, 4096 random voxels inside one 64^3 cube, a ball of radius 32
cleared) are written and undone over and over, so the scene stays the builder's while the array fills with garbage, until the
garbage exceeds the live tree; then the tree is compacted.  Per repetition: the call's wall time and the device time of its
kernels (vrc_compact_info.seconds), the words before and after, and the peak of the device memory in use during the call (a
thread polls the free memory while the call runs).  Then the frame time (1920 x 1080, the scene header's camera, one light,
hit records off, after vrc_prepare has rebuilt the table and the boxes) on three trees that hold the same scene: (a) the edited
tree, (b) the compacted tree, (c) a tree built fresh by the device builder.  Each figure: the median and the spread (min .. max)
of --reps repetitions after 2 warm-ups.  Usage: python tools/compact_rate.py [--reps 7] [--depth 12] [--out FILE]"""
import argparse
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bench
import edit_rate
import voxel_raycaster_amd as vrc

W, H, FRAMES = 1920, 1080, 20


def stat(v):
    return f"{np.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


class Batches:
    """the three batches on the device, with the materials they find and the ones they write"""
    def __init__(self, c, depth):
        self.legs = []
        for name, p in edit_rate.batches(np.random.default_rng(1), depth).items():
            n = len(p)
            tp = torch.from_numpy(p).to("cuda:0")
            before = torch.empty(n, dtype=torch.int32, device="cuda:0")
            assert c.get_voxels_device(tp.data_ptr(), n, before.data_ptr()), c.last_error()
            new = torch.where(before != 0, 0, 5).to(torch.int32) if name.startswith("random") else torch.zeros_like(before)
            self.legs.append((tp, before, new, n))

    def round(self, c):
        """every batch written and undone: the scene is what it was, the array has grown"""
        for tp, before, new, n in self.legs:
            assert c.set_voxels_device(tp.data_ptr(), new.data_ptr(), n)["voxels_changed"] > 0
            c.set_voxels_device(tp.data_ptr(), before.data_ptr(), n)


def fill_with_garbage(c, batches, live):
    rounds = 0
    while c.octree_size()[0] <= 2 * live:
        batches.round(c)
        rounds += 1
    return rounds


def polled_compact(c):
    """(info, wall ms, bytes in use before, peak bytes in use during the call)"""
    torch.cuda.synchronize()
    free0, total = torch.cuda.mem_get_info(0)
    low, stop = [free0], threading.Event()

    def poll():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(0)[0])

    t = threading.Thread(target=poll)
    t.start()
    t0 = time.perf_counter()
    info = c.compact_octree()
    t1 = time.perf_counter()
    stop.set()
    t.join()
    return info, 1e3 * (t1 - t0), total - free0, total - low[0]


def frame_ms(c):
    """[ms per frame] of FRAMES frames, the table and the boxes in place"""
    assert c.prepare(), c.last_error()
    for _ in range(5):
        assert c.compute(), c.last_error()
    out = []
    for _ in range(FRAMES):
        c.timing_reset()
        assert c.compute(), c.last_error()
        n, ms = c.timing()
        out.append(ms / max(n, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"# tools/compact_rate.py: {torch.cuda.get_device_name(0)}; depth {args.depth}; median (min .. max) of {args.reps} repetitions after 2 warm-ups",
             "# every repetition: the three batches of tools/edit_rate.py written and undone until the array is more than twice the live tree, then vrc_compact_octree"]
    sc = bench.device_scene_header(args.depth)
    c = bench.make_caster(sc, W, H, 0, hit_records=0)
    n_built = c.octree_size()[0]
    batches = Batches(c, args.depth)
    live = c.compact_octree(dry_run=True)["n_descriptors"]
    lines.append(f"builder's tree: {n_built} words; its compacted size {live} words")
    wall, dev, peak, edited_frames, info, rounds = [], [], [], None, None, 0
    for k in range(args.reps + 2):
        rounds = fill_with_garbage(c, batches, live)
        if k == 0:
            edited_frames = frame_ms(c)                         # (a): garbage, the bricks' stride and far pointers into old arrays
        dry = c.compact_octree(dry_run=True)
        info, ms, used0, used_peak = polled_compact(c)
        assert {a: b for a, b in dry.items() if a != "seconds"} == {a: b for a, b in info.items() if a != "seconds"}
        live = info["n_descriptors"]
        if k >= 2:
            wall.append(ms); dev.append(1e3 * info["seconds"]); peak.append((used_peak - used0) / 2 ** 20)
    lines.append(f"edit rounds per repetition (three batches, written and undone): {rounds}")
    lines.append(f"words before {info['descriptors_before']}  after {info['n_descriptors']} (far slots {info['far_slots']})  "
                 f"attachment slots before {info['attachments_before']}  after {info['n_attachments']}")
    lines.append(f"vrc_compact_octree call ms        {stat(wall)}")
    lines.append(f"vrc_compact_info.seconds ms       {stat(dev)}")
    lines.append(f"device memory above the level before the call, peak MiB  {stat(peak)}   octree_bytes after {c.memory_usage2()['octree_bytes']}")
    compacted_frames = frame_ms(c)                              # (b)
    f = bench.make_caster(sc, W, H, 0, hit_records=0)
    fresh_frames = frame_ms(f)                                  # (c)
    same = torch.equal(torch.from_numpy(c.read_image().view(np.uint32).copy()), torch.from_numpy(f.read_image().view(np.uint32).copy()))
    lines.append(f"frame ms, {W} x {H}, {FRAMES} frames: (a) edited tree      {stat(edited_frames)}")
    lines.append(f"frame ms, {W} x {H}, {FRAMES} frames: (b) compacted tree   {stat(compacted_frames)}")
    lines.append(f"frame ms, {W} x {H}, {FRAMES} frames: (c) builder's tree   {stat(fresh_frames)}")
    lines.append(f"frames of (b) and (c) bit-identical: {same}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
