#!/usr/bin/env python
"""Time one 1024^2 turntable frame of every video type on the GPU: HIP events around rasterise + shade (what export_orbit_video enqueues per
frame, without the device-to-host copy), median of --iters after --warmup, the rgb frame (utx_texture_shade) in the same process and
alternating with the geometry types, on a 20 k-face mesh with a 2048^2 texture.  Prints one line per type and the ratio to rgb.

    python tools/time_video_types.py [--size 1024] [--faces 20000] [--iters 30] [--warmup 5]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--faces", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU fall-back to time"
    from unitex_amd.texturetools import camera, meshes, ops
    verts, faces, uvs = meshes.sphere_with_faces(a.faces)
    dev, S = "cuda:0", a.size
    vd = torch.from_numpy(verts).to(dev).contiguous()
    fd = torch.from_numpy(faces).to(dev, torch.int32).contiguous()
    uvd = torch.from_numpy(uvs).to(dev).contiguous()
    nd = torch.nn.functional.normalize(vd, dim=-1).contiguous()
    tex = torch.rand(2048, 2048, 3, generator=torch.Generator().manual_seed(0)).to(dev).contiguous()
    c2ws = camera.generate_orbit_views_c2ws(9, radius=2.8, height=0.0, theta_0=0.0, degree=True)[:8].float().contiguous()
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    mvp = torch.matmul(camera.intr_to_proj(intr, perspective=True), camera.c2w_to_w2c(c2ws)).to(dev).contiguous()
    clip, _ = ops.transform_points(vd, mvp, want_ndc=False)
    cam, _ = ops.transform_points(vd, camera.c2w_to_w2c(c2ws).to(dev).contiguous(), want_ndc=False)
    ncam = ops.camera_normals(nd, c2ws.to(dev))
    attr = {"world_normal": lambda i: nd, "camera_normal": lambda i: ncam[i], "world_position": lambda i: vd,
            "camera_position": lambda i: cam[i, :, :3], "z_depth": lambda i: clip[i, :, 3:], "distance": lambda i: cam[i, :, :3]}
    r0 = ops.rasterize(clip[0].contiguous(), fd, S, S)
    scale = {t: ops.gbuffer_range(t, r0, fd, attr[t](0))[:2] for t in ("z_depth", "distance")}

    def frame(t, i):
        rast = ops.rasterize(clip[i].contiguous(), fd, S, S)
        if t == "rgb":
            return ops.texture_shade(rast, uvd, fd, tex, bg=(1.0, 1.0, 1.0))
        return ops.gbuffer_shade(t, rast, fd, attr[t](i), scale2=scale.get(t), ndc=t not in scale, bg=(1.0, 1.0, 1.0))
    types = ["rgb"] + list(attr)
    times = {t: [] for t in types}
    for it in range(a.warmup + a.iters):
        for t in types:                      # alternate the types inside every round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            frame(t, it % 8)
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[t].append(e0.elapsed_time(e1))
    print("device %s, %d^2, %d faces, median of %d (min .. max) ms per frame, rasterise + shade" % (torch.cuda.get_device_name(0), S, faces.shape[0], a.iters))
    base = float(np.median(times["rgb"]))
    for t in types:
        x = np.asarray(times[t])
        print("%-16s %.4f (%.4f .. %.4f)  ratio to rgb %.3f" % (t, np.median(x), x.min(), x.max(), np.median(x) / base))


if __name__ == "__main__":
    main()
