#!/usr/bin/env python
"""Device time of one lit turntable frame without and with a tangent-space normal map (reported in DESIGN.md 8 and the README, not gated):
utx_pbr_shade and utx_pbr_shade_nm on the same --size^2 raster of the --faces benchmark sphere, in the same process, interleaved (A B A B ...), timed
with events after --warmup rounds; medians of --iters and their ratio.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=50000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--tex", type=int, default=2048)
    ap.add_argument("--cube-res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from unitex_amd.texturetools import camera, meshes, ops
    from unitex_amd.texturetools.video import _vertex_normals
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    verts, faces, uvs = meshes.sphere_with_faces(a.faces)
    nrm = _vertex_normals(torch.from_numpy(verts), torch.from_numpy(faces), "angle")
    tng = meshes.vertex_tangents(verts, faces, uvs, nrm)
    vd, fd, uvd, nd, td = (torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(uvs).to(dev), nrm.to(dev), tng.to(dev))
    fn = ops.face_normals(vd, fd)
    tex = lambda: torch.from_numpy(rng.uniform(0, 1, (a.tex, a.tex, 3)).astype(np.float32)).to(dev)
    kd, ks, nm = tex(), tex(), tex()
    N = a.cube_res
    ld, ls = (torch.from_numpy(rng.uniform(0, 4, (6, N, N, 3)).astype(np.float32)).to(dev) for _ in range(2))
    lut = ops.dfg_lut(256, 1024, dev)
    c2w = camera.generate_orbit_views_c2ws(2, radius=2.8, height=0.0, theta_0=0.0, degree=True)[:1]
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    mvp = torch.matmul(camera.intr_to_proj(intr, perspective=True), camera.c2w_to_w2c(c2w)).to(dev).contiguous()
    clip, _ = ops.transform_points(vd, mvp, want_ndc=False)
    rast = ops.rasterize(clip[0].contiguous(), fd, a.size, a.size)
    eye = c2w[0, :3, 3].tolist()
    plain = lambda: ops.pbr_shade(rast, fd, vd, nd, uvd, kd, ks, eye, ld, ls, lut)
    mapped = lambda: ops.pbr_shade(rast, fd, vd, nd, uvd, kd, ks, eye, ld, ls, lut, v_tng=td, f_nrm=fn, normal_map=nm)
    times = {"pbr_shade_ms": [], "pbr_shade_nm_ms": []}
    for it in range(a.warmup + a.iters):
        for key, fn_ in (("pbr_shade_ms", plain), ("pbr_shade_nm_ms", mapped)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn_()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[key].append(e0.elapsed_time(e1))
    res = {"faces": int(faces.shape[0]), "size": a.size, "tex": a.tex, "cube_res": N, "covered": float((rast[..., 3] > 0).float().mean()), "iters": a.iters}
    for k, v in times.items():
        res[k] = float(np.median(v))
        res[k.replace("_ms", "_min_ms")] = float(np.min(v))
    res["ratio"] = res["pbr_shade_nm_ms"] / res["pbr_shade_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
