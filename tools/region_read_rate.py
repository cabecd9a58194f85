"""Region-read rates (vrc_read_regions_device, csrc/voxel_read.hip): output bytes per second for (a) 4096 surface chunks of 32^3
on the map's 32-voxel chunk grid in the depth-12 device-built bench scene, coarse table built by validate, and (b) the whole of
a 512^3 scene built by vrc_build_dense_grid from the resident map (the depth-9 shell terrain with material attachments), in the
SVO branch and in the array branch.  Beside each leg, in the same run: a device-to-device hipMemcpy of the same byte count (the
floor: the output alone, written once) and vrc_box_intersection_device listing the same regions with max_voxels = V (what a host
had to use before: 16 bytes per solid voxel, Morton order).  Each figure: hip events around the call, the median of --reps calls
after 2 warm-ups.  Usage: python tools/region_read_rate.py [--reps 10] [--out FILE]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import bench
import voxel_raycaster_amd as vrc


def timed(call, reps):
    """Median device milliseconds of call() (work that is on the null stream or waits for it) after 2 warm-ups."""
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def surface_chunks(rng, depth, n, edge):
    """n distinct chunks of edge^3 on the map's chunk grid that hold the surface (shell_column hi) at their centre column."""
    dim = 1 << depth
    cells = dim // edge
    pick = rng.choice(cells * cells, size=n, replace=False)
    cx, cy = pick % cells, pick // cells
    hi = np.array([vrc.shell_column(depth, int(x * edge + edge // 2), int(y * edge + edge // 2))[1] for x, y in zip(cx, cy)])
    return np.stack([cx * edge, cy * edge, (hi // edge) * edge], axis=1).astype(np.int32)


def leg(c, hip, name, lo, size, reps, lines):
    n = len(lo)
    volume = int(size[0]) * int(size[1]) * int(size[2])
    total = n * volume
    tl = torch.from_numpy(np.ascontiguousarray(lo, dtype=np.int32)).to("cuda:0")
    out = torch.empty((total,), dtype=torch.int8, device="cuda:0")

    def read():
        assert c.read_regions_device(tl.data_ptr(), n, size, out.data_ptr(), total), c.last_error()
    read_ms = timed(read, reps)
    solid = int(torch.count_nonzero(out).item())
    src = torch.zeros((total,), dtype=torch.int8, device="cuda:0")

    def copy():
        assert hip.hipMemcpyDtoDAsync(ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(src.data_ptr()), ctypes.c_size_t(total), None) == 0
    copy_ms = timed(copy, reps)
    del src
    boxes = np.concatenate([lo, np.broadcast_to(np.asarray(size, np.int32), (n, 3))], axis=1).astype(np.float32)
    tb = torch.from_numpy(boxes).to("cuda:0")
    rec = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
    cnt = torch.empty((n,), dtype=torch.int64, device="cuda:0")
    vox = torch.empty((n, volume, 4), dtype=torch.int32, device="cuda:0")

    def listed():
        assert c.box_intersection_device(tb.data_ptr(), n, rec.data_ptr(), cnt.data_ptr(), vox.data_ptr(), volume), c.last_error()
    box_ms = timed(listed, reps)
    assert int(cnt.sum().item()) == solid, "the box query counts other voxels than the read returns"
    del vox
    lines.append(f"{name:22s} {n:6d} {size[0]:4d}x{size[1]}x{size[2]} {total:12d} {solid:11d} {read_ms:9.3f} {total / read_ms / 1e6:9.2f} "
                 f"{copy_ms:9.3f} {total / copy_ms / 1e6:9.2f} {box_ms:10.3f}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    hip = ctypes.CDLL("libamdhip64.so")
    rng = np.random.default_rng(1)
    lines = [f"# tools/region_read_rate.py: {torch.cuda.get_device_name(0)}; median of {args.reps} calls after 2 warm-ups (hip events)",
             "# read = vrc_read_regions_device; copy = hipMemcpyDtoDAsync of the same bytes (the floor); list = vrc_box_intersection_device,",
             "# max_voxels = V, on the same regions (16 bytes per solid voxel)",
             "# leg  regions  size  output bytes  solid voxels  read ms  read GB/s  copy ms  copy GB/s  list ms"]
    # (a) surface chunks of the depth-12 shell terrain
    depth = 12
    sc = bench.device_scene_header(depth)
    c = bench.make_caster(sc, 256, 144, 0)
    leg(c, hip, "a_surface_chunks_d12", surface_chunks(rng, depth, 4096, 32), (32, 32, 32), args.reps, lines)
    del c
    # (b) the whole of a 512^3 dense-grid scene, both branches
    depth, dim = 9, 512
    grid = vrc.shell_terrain_dense(depth, seed=1, thickness=2)
    sc = dict(bench.device_scene_header(depth))
    c = vrc.CLCaster()
    assert c.init(0)
    ok = (c.add_to_settings_buffer("octree_dimensions", "OCTDIM", dim) and c.add_to_settings_buffer("using_octree", "OCTENABLED", 0)
          and c.add_to_settings_buffer("max_distance", "MAX_DISTANCE", 3 * dim) and c.assign_map(grid, (dim, dim, dim)))
    assert ok, c.last_error()
    c.build_dense_grid(depth, None, attachments=True)
    ok = (c.assign_camera(sc["cam_dir"], sc["cam_pos"]) and c.create_viewport(256, 144) and c.assign_lights(sc["lights"])
          and c.create_texture_atlas(sc["atlas"], (16, 16)) and c.validate())
    assert ok, c.last_error()
    whole = np.zeros((1, 3), np.int32)
    leg(c, hip, "b_whole_512_svo", whole, (dim, dim, dim), args.reps, lines)
    assert c.overwrite_setting("using_octree", 1) and c.validate(), c.last_error()
    leg(c, hip, "b_whole_512_array", whole, (dim, dim, dim), args.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
