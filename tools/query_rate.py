"""Ray-query rates (vrc_cast_rays_device, csrc/raycast_query.hip) on the depth-12 bench scene: (a) the headline camera's 1920 x 1080
pixel rays with AS_PIXEL, (b) 4 M random rays to the map's edge, (c) 1 M straight-down rays from random (x, y).  Each leg is timed
with hip events around the device-pointer call (after a warm-up), with the coarse table and the empty boxes on and off, and the
host-array call as a PCIe-inclusive rate.  Usage: python tools/query_rate.py [--depth 12] [--reps 10] [--out FILE]"""
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
from oracle import orc

F = np.float32


def pixel_rays(sc, w, h):
    """The headline frame's primary rays: the reference viewport table rotated with the frame's trig, as ray_setup does."""
    vp = orc.create_viewport(w, h)
    s1, c1, s2, c2 = (F(v) for v in orc.camera_trig(np.asarray(sc["cam_dir"], F)))
    px, py, pz = vp[..., 0], vp[..., 1], vp[..., 2]
    x, y, z = pz * s1 + px * c1, py, pz * c1 - px * s1
    d = np.stack([x * c2 - y * s2, x * s2 + y * c2, z], axis=-1).reshape(-1, 3)
    return np.concatenate([np.broadcast_to(np.asarray(sc["cam_pos"], F), d.shape), d], axis=1).astype(F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sc = bench.build_scene(args.depth)
    dim, w, h = sc["dim"], 1920, 1080
    c = bench.make_caster(sc, w, h, 0)
    assert c.add_to_settings_buffer("coarse_log2", "COARSE_LOG2", -1) and c.add_to_settings_buffer("empty_boxes", "EMPTY_BOXES", -1)
    assert c.validate(), c.last_error()
    assert c.compute(), c.last_error()
    frame_ms = c.timing()[1] / max(1, c.timing()[0])
    rng = np.random.default_rng(1)
    legs = {}
    legs["a_pixels_as_pixel"] = (pixel_rays(sc, w, h), 3 * dim, True)
    o = rng.uniform(0, dim, size=(4 << 20, 3)).astype(F)
    d = rng.normal(size=(4 << 20, 3)).astype(F)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    legs["b_random_to_edge"] = (np.concatenate([o, d], axis=1), 0, False)
    o = np.stack([rng.uniform(0, dim, 1 << 20), rng.uniform(0, dim, 1 << 20), np.full(1 << 20, dim - 0.5)], axis=1).astype(F)
    d = np.tile(np.array([0, 0, -1], F), (1 << 20, 1))
    legs["c_straight_down"] = (np.concatenate([o, d], axis=1), 0, False)
    lines = [f"# tools/query_rate.py: depth {args.depth} bench scene, {torch.cuda.get_device_name(0)}; headline frame (1920x1080, "
             f"1 light, shadow rays) {frame_ms:.3f} ms kernel time for comparison", "# leg  rays  structures  device ms  Mrays/s  "
             "(host path incl. PCIe: ms, Mrays/s)  hits  left_map  mean steps"]
    for name, (rays, max_steps, as_pixel) in legs.items():
        n = len(rays)
        rt = torch.from_numpy(np.ascontiguousarray(rays)).to("cuda:0")
        out = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
        for boxes, table in ((-1, -1), (0, -1), (0, 0)):
            assert c.overwrite_setting("empty_boxes", boxes) and c.overwrite_setting("coarse_log2", table)
            for _ in range(2):                                     # warm-up
                assert c.cast_rays_device(rt.data_ptr(), out.data_ptr(), n, max_steps, as_pixel), c.last_error()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                assert c.cast_rays_device(rt.data_ptr(), out.data_ptr(), n, max_steps, as_pixel)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            dev_ms = float(np.median(ms))
            rec = out.cpu().numpy()
            t0 = time.perf_counter()
            host = c.cast_rays(rays, max_steps=max_steps, as_pixel=as_pixel)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(host, rec)
            what = {(-1, -1): "table+boxes", (0, -1): "table", (0, 0): "none"}[(boxes, table)]
            lines.append(f"{name:20s} {n:8d}  {what:12s} {dev_ms:9.3f}  {n / dev_ms / 1e3:8.1f}  ({host_ms:8.1f}, {n / host_ms / 1e3:7.1f})  "
                         f"{int((rec[:, 5] == 1).sum()):8d} {int((rec[:, 5] == 2).sum()):8d}  {rec[:, 6].mean():8.1f}")
            print(lines[-1], flush=True)
    assert c.overwrite_setting("empty_boxes", -1) and c.overwrite_setting("coarse_log2", -1)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
