"""Face-extraction rates (vrc_extract_faces_device, csrc/face_extract.hip) on the legs of tools/region_read_rate.py: (a) 4096
surface chunks of 32^3 on the map's 32-voxel chunk grid in the depth-12 device-built bench scene, coarse table built by validate,
and (b) the whole of a 512^3 scene built by vrc_build_dense_grid from the resident map (the depth-9 shell terrain with material
attachments), in the SVO branch and in the array branch.  Per leg: the faces, their bytes and the solid voxels; the count-only
call and the count + emit call (capacity = the total), each as hip events around the call, as the call's own kernel time
(vrc_faces_info.seconds) and as host wall time; and, in the same run, the two routes a mesher had before: vrc_read_regions_device
of the same chunks with a one-voxel apron and vrc_box_intersection_device with a full list.  Each figure: the median of --reps
calls after 2 warm-ups.  Usage: python tools/face_extract_rate.py [--reps 10] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import bench
import voxel_raycaster_amd as vrc
from region_read_rate import surface_chunks, timed


def timed_call(call, reps):
    """(hip-event ms, the call's own kernel ms, host wall ms): medians over reps calls after 2 warm-ups; call() returns the info dict."""
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ev, own, wall = [], [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        info = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
        own.append(info["seconds"] * 1e3)
    return float(np.median(ev)), float(np.median(own)), float(np.median(wall))


def leg(c, name, lo, size, reps, lines):
    n = len(lo)
    size = tuple(int(v) for v in size)
    volume = size[0] * size[1] * size[2]
    lo = np.ascontiguousarray(lo, dtype=np.int32)
    tl = torch.from_numpy(lo).to("cuda:0")
    cnt = torch.empty((n,), dtype=torch.int64, device="cuda:0")
    total = c.extract_faces_device(tl.data_ptr(), n, size, cnt.data_ptr())["faces_total"]
    faces = torch.empty((max(total, 1), 4), dtype=torch.int32, device="cuda:0")
    count_ms = timed_call(lambda: c.extract_faces_device(tl.data_ptr(), n, size, cnt.data_ptr()), reps)
    emit_ms = timed_call(lambda: c.extract_faces_device(tl.data_ptr(), n, size, cnt.data_ptr(), faces.data_ptr(), total), reps)
    assert int(cnt.sum().item()) == total
    inner = c.extract_faces_device(tl.data_ptr(), n, size, cnt.data_ptr(), no_map_edge=True)["faces_total"]
    # route 1: the same chunks with a one-voxel apron, read densely (the faces are then found on the host)
    apron = tuple(v + 2 for v in size)
    apron_bytes = n * apron[0] * apron[1] * apron[2]
    ta = torch.from_numpy(lo - 1).to("cuda:0")
    out = torch.empty((apron_bytes,), dtype=torch.int8, device="cuda:0")

    def read():
        assert c.read_regions_device(ta.data_ptr(), n, apron, out.data_ptr(), apron_bytes), c.last_error()
    read_ms = timed(read, reps)
    del out
    # route 2: the solid voxels of the same chunks as a list (16 bytes each, Morton order; buried and surface voxels alike)
    boxes = np.concatenate([lo, np.broadcast_to(np.asarray(size, np.int32), (n, 3))], axis=1).astype(np.float32)
    tb = torch.from_numpy(boxes).to("cuda:0")
    rec = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
    bcnt = torch.empty((n,), dtype=torch.int64, device="cuda:0")
    vox = torch.empty((n, volume, 4), dtype=torch.int32, device="cuda:0")

    def listed():
        assert c.box_intersection_device(tb.data_ptr(), n, rec.data_ptr(), bcnt.data_ptr(), vox.data_ptr(), volume), c.last_error()
    list_ms = timed(listed, reps)
    solid = int(bcnt.sum().item())
    del vox
    lines.append(f"{name:22s} {n:6d} {size[0]:4d}x{size[1]}x{size[2]} {solid:11d} {total:10d} {inner:10d} {16 * total:11d} "
                 f"{count_ms[0]:8.3f} {count_ms[1]:8.3f} {count_ms[2]:8.3f} {emit_ms[0]:8.3f} {emit_ms[1]:8.3f} {emit_ms[2]:8.3f} "
                 f"{apron_bytes:11d} {read_ms:8.3f} {16 * solid:11d} {list_ms:8.3f}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    lines = [f"# tools/face_extract_rate.py: {torch.cuda.get_device_name(0)}; median of {args.reps} calls after 2 warm-ups, milliseconds",
             "# count = vrc_extract_faces_device with capacity 0; emit = the same call with capacity = faces (count + emit passes);",
             "# ev = hip events around the call, krn = vrc_faces_info.seconds (the call's kernels), host = wall time of the call;",
             "# no-edge = the faces with VRC_FACES_NO_MAP_EDGE; apron read = vrc_read_regions_device of the same chunks grown by one",
             "# voxel on every side; list = vrc_box_intersection_device, max_voxels = V, on the same chunks (16 bytes per solid voxel)",
             "# leg  regions  size  solid voxels  faces  no-edge faces  face bytes  count ev  count krn  count host  emit ev  emit krn  "
             "emit host  apron bytes  apron read ms  list bytes  list ms"]
    depth = 12
    sc = bench.device_scene_header(depth)
    c = bench.make_caster(sc, 256, 144, 0)
    leg(c, "a_surface_chunks_d12", surface_chunks(rng, depth, 4096, 32), (32, 32, 32), args.reps, lines)
    del c
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
    leg(c, "b_whole_512_svo", whole, (dim, dim, dim), args.reps, lines)
    assert c.overwrite_setting("using_octree", 1) and c.validate(), c.last_error()
    leg(c, "b_whole_512_array", whole, (dim, dim, dim), args.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
