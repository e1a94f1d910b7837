#!/usr/bin/env python
"""Times of the image-based PBR path on one GPU (reported in DESIGN.md 8, not gated):
  * the one-time prefilters at --cube-res (lat-long conversion, diffuse = 6 N^2 outputs x 6 N^2 inputs, specular at roughness 0.08 / cutoff 0.99) and the
    256^2 split-sum table;
  * one --size^2 utx_pbr_shade frame beside the unlit rgb frame (utx_texture_shade) of the same raster, in the same process: device time by events,
    median of --iters after --warmup.
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cube-res", type=int, default=512)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from unitex_amd.texturetools import camera, ops
    from unitex_amd.texturetools.pbr import ndf_cutoff
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lat = torch.from_numpy(rng.uniform(0, 4, (256, 512, 3)).astype(np.float32)).to(dev)
    N = a.cube_res
    cut = ndf_cutoff(0.08, 0.99)
    texels, tiles = ops.cubemap_tables(N, cut, dev)
    cube = ops.latlong_to_cubemap(lat, N)
    res = {"cube_res": N, "costheta_cutoff": cut}
    res["latlong_ms"] = _time(lambda: ops.latlong_to_cubemap(lat, N), 1, 3)
    res["diffuse_ms"] = _time(lambda: ops.cubemap_diffuse(cube, texels), 1, 2)
    res["specular_ms"] = _time(lambda: ops.cubemap_specular(cube, 0.08, cut, texels, tiles), 1, 3)
    res["dfg_lut_256_1024_ms"] = _time(lambda: ops.dfg_lut(256, 1024, dev), 1, 3)
    ld, ls, lut = ops.cubemap_diffuse(cube, texels), ops.cubemap_specular(cube, 0.08, cut, texels, tiles), ops.dfg_lut(256, 1024, dev)
    # a UV sphere that fills most of the frame
    nu, nv = 256, 128
    u, v = np.meshgrid(np.arange(nu + 1) / nu, np.arange(nv + 1) / nv, indexing="ij")
    th, ph = v * np.pi, u * 2 * np.pi
    p = np.stack([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda i, j: i * (nv + 1) + j
    faces = np.asarray([[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i in range(nu) for j in range(nv)] +
                       [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(nu) for j in range(nv)], np.int32)
    uv = np.stack([u, v], -1).reshape(-1, 2).astype(np.float32)
    vd, nd, fd, uvd = torch.from_numpy(p).to(dev), torch.from_numpy(p.copy()).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(uv).to(dev)
    kd = torch.from_numpy(rng.uniform(0, 1, (2048, 2048, 3)).astype(np.float32)).to(dev)
    ks = torch.from_numpy(rng.uniform(0, 1, (2048, 2048, 3)).astype(np.float32)).to(dev)
    c2w = camera.generate_orbit_views_c2ws(2, radius=2.8, height=0.0, theta_0=0.0, degree=True)[:1]
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    mvp = torch.matmul(camera.intr_to_proj(intr, perspective=True), camera.c2w_to_w2c(c2w)).to(dev).contiguous()
    clip, _ = ops.transform_points(vd, mvp, want_ndc=False)
    rast = ops.rasterize(clip[0].contiguous(), fd, a.size, a.size)
    eye = c2w[0, :3, 3].tolist()
    res["size"] = a.size
    res["covered"] = float((rast[..., 3] > 0).float().mean())
    res["rgb_unlit_ms"] = _time(lambda: ops.texture_shade(rast, uvd, fd, kd), a.warmup, a.iters)
    res["pbr_shade_ms"] = _time(lambda: ops.pbr_shade(rast, fd, vd, nd, uvd, kd, ks, eye, ld, ls, lut), a.warmup, a.iters)
    res["pbr_shade_default_ks_ms"] = _time(lambda: ops.pbr_shade(rast, fd, vd, nd, uvd, kd, None, eye, ld, ls, lut), a.warmup, a.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
