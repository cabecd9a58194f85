"""Edit rates (vrc_set_voxels_device, csrc/voxel_edit.hip) on the depth-12 device-built bench scene -- a tree that exists only in
HBM -- for three batches at the terrain's surface: one voxel, 4096 random voxels inside one 64^3 cube, a solid ball of radius
32 cleared.  Per batch: the call's wall time and the device time of its kernels (vrc_edit_info.seconds), what the array grew
by, and the vrc_prepare that follows -- first with empty_boxes = 0 (the coarse table alone), then with the default (the empty
boxes on top).  Every repetition edits voxels that differ from the scene (the batch is undone, untimed, before the next one).
Beside it the only route the library had before: vrc_read_regions_device of the whole map, the change on the grid, then
vrc_assign_map + vrc_build_dense_grid from the resident map.  That route moves dim^3 bytes, 64 GiB at depth 12, so it is run on
the depth-9 scene (128 MiB), together with the same three batches there.  Each figure: the median and the spread (min .. max)
of --reps repetitions after 2 warm-ups.  Usage: python tools/edit_rate.py [--reps 7] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import bench
import voxel_raycaster_amd as vrc


def stat(ms):
    return f"{np.median(ms):9.3f} ({min(ms):.3f} .. {max(ms):.3f})"


def batches(rng, depth):
    """{name: positions (n, 3) int32} around the surface above the map's centre column"""
    dim = 1 << depth
    cx = cy = dim // 2
    _, hi = vrc.shell_column(depth, cx, cy)
    one = np.array([[cx, cy, hi]], np.int32)
    cube = (np.array([cx - 32, cy - 32, hi - 40]) + rng.integers(0, 64, size=(4096, 3))).astype(np.int32)
    g = np.arange(-32, 33)
    off = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    ball = (np.array([cx, cy, hi - 16]) + off[(off ** 2).sum(axis=1) <= 32 * 32]).astype(np.int32)
    return {"one_voxel": one, "random_4096_in_64^3": cube, "ball_r32_cleared": ball}


def edit_legs(c, depth, reps, lines):
    rng = np.random.default_rng(1)
    for name, p in batches(rng, depth).items():
        n = len(p)
        tp = torch.from_numpy(p).to("cuda:0")
        before = torch.empty(n, dtype=torch.int32, device="cuda:0")
        assert c.get_voxels_device(tp.data_ptr(), n, before.data_ptr()), c.last_error()
        # what the batch writes: the ball and the single voxel clear, the random batch toggles between empty and 5
        new = torch.where(before != 0, 0, 5).to(torch.int32) if name.startswith("random") else torch.zeros_like(before)
        wall, dev, table, boxes, info = [], [], [], [], None
        for k in range(reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = c.set_voxels_device(tp.data_ptr(), new.data_ptr(), n)
            t1 = time.perf_counter()
            assert c.add_to_settings_buffer("empty_boxes", "EMPTY_BOXES", 0) and c.prepare(), c.last_error()
            t2 = time.perf_counter()
            assert c.add_to_settings_buffer("empty_boxes", "EMPTY_BOXES", -1) and c.prepare(), c.last_error()
            t3 = time.perf_counter()
            assert info["voxels_changed"] > 0
            mem = c.memory_usage2()
            assert mem["coarse_bytes"] > 0 and mem["box_bytes"] > 0, mem
            c.set_voxels_device(tp.data_ptr(), before.data_ptr(), n)               # undo (untimed)
            if k >= 2:
                wall.append(1e3 * (t1 - t0)); dev.append(1e3 * info["seconds"]); table.append(1e3 * (t2 - t1)); boxes.append(1e3 * (t3 - t2))
        lines.append(f"d{depth}_{name:22s} {n:7d} {info['voxels_changed']:8d} {info['bricks_touched']:6d} {info['descriptors_added']:9d} "
                     f"{stat(wall)} {stat(dev)} {stat(table)} {stat(boxes)}")
        print(lines[-1], flush=True)


def baseline(c, depth, reps, lines):
    """read the whole map to the host, change it there (one voxel), assign it as the map again and build the tree from it"""
    dim = 1 << depth
    lo = torch.zeros((1, 3), dtype=torch.int32, device="cuda:0")
    out = torch.empty(dim ** 3, dtype=torch.int8, device="cuda:0")
    read, build = [], []
    for k in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert c.read_regions_device(lo.data_ptr(), 1, (dim,) * 3, out.data_ptr(), out.numel()), c.last_error()
        host = out.cpu().numpy()                                    # vrc_assign_map takes the host's array
        t1 = time.perf_counter()
        host[(k * 7919) % host.size] ^= 5
        assert c.assign_map(host, (dim,) * 3), c.last_error()
        c.build_dense_grid(depth, None, attachments=True)
        assert c.validate(), c.last_error()
        t2 = time.perf_counter()
        if k >= 2:
            read.append(1e3 * (t1 - t0)); build.append(1e3 * (t2 - t1))
    lines.append(f"d{depth}_baseline_read_whole_map_to_host ms {stat(read)}   assign_map + build_dense_grid + validate ms {stat(build)}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"# tools/edit_rate.py: {torch.cuda.get_device_name(0)}; median (min .. max) of {args.reps} repetitions after 2 warm-ups, milliseconds",
             "# call = wall time of vrc_set_voxels_device; kernels = vrc_edit_info.seconds; table / boxes = the vrc_prepare that follows with",
             "# empty_boxes = 0, then the default on top.  baseline: the route before this call existed (see the file's docstring)",
             "# leg  edits  voxels changed  bricks  words added  call ms  kernels ms  prepare: table ms  prepare: boxes ms"]
    for depth in (12, 9):
        sc = bench.device_scene_header(depth)
        c = bench.make_caster(sc, 256, 144, 0)
        n0 = c.octree_size()[0]
        edit_legs(c, depth, args.reps, lines)
        lines.append(f"d{depth}_tree: {n0} descriptors before, {c.octree_size()[0]} after {3 * 2 * (args.reps + 2)} edits; octree_bytes {c.memory_usage2()['octree_bytes']}")
        if depth == 9:
            baseline(c, depth, args.reps, lines)
        del c
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
