#!/usr/bin/env python
"""Device time of the atlas-space geometry buffers (reported in DESIGN.md 8, not gated): utx_uv_gbuffer, every buffer of --views cameras in one
launch, against what a caller had to write before it -- one ops.interpolate per view and attribute plus torch for the normalisations, norms,
dot product and background selects -- on the same --size^2 UV raster of the --faces benchmark sphere and the same per-view per-vertex arrays,
in the same process, interleaved (A B A B ...), timed with events after --warmup rounds; medians of --iters and their ratio.  Both sides
allocate their outputs inside the timed region (the caching allocator serves them after the warm-up).  Prints one JSON line."""
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
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from unitex_amd.texturetools import camera, meshes, ops
    from unitex_amd.texturetools.video import _vertex_normals
    dev = torch.device("cuda:0")
    verts, faces, uvs = meshes.sphere_with_faces(a.faces)
    nrm = _vertex_normals(torch.from_numpy(verts), torch.from_numpy(faces), "area").float()
    vd, fd, nd = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), nrm.to(dev).contiguous()
    uv = torch.from_numpy(uvs).to(dev) * 2.0 - 1.0
    rast = ops.rasterize(torch.cat([uv, torch.zeros_like(uv[:, :1]), torch.ones_like(uv[:, :1])], -1).contiguous(), fd, a.size, a.size)
    c2ws = camera.generate_orbit_views_c2ws(a.views + 1, radius=2.8, height=0.0, theta_0=0.0, degree=True)[:a.views].float()
    pcam = ops.transform_points(vd, camera.c2w_to_w2c(c2ws).to(dev).contiguous(), want_ndc=False)[0][..., :3].contiguous()
    ncam = ops.camera_normals(nd, c2ws.to(dev).contiguous())
    want = tuple(ops.UV_GBUFFERS)
    cov = (rast[..., 3] > 0)[..., None]

    def fused():
        return ops.uv_gbuffer(rast, fd, vd, nd, want=want, v_pos_cam=pcam, v_nrm_cam=ncam)

    def unit(x):
        return x / torch.sqrt((x * x).sum(-1, keepdim=True)).clamp_min(1e-12)

    def composed():
        sel = lambda x, fill: torch.where(cov, x, torch.full_like(x, fill))
        out = {"mask": cov[..., 0].to(torch.uint8), "alpha": cov.float(),
               "world_normal": sel(unit(ops.interpolate(nd, rast, fd)), -1.0)[None], "world_position": sel(ops.interpolate(vd, rast, fd), -1.0)[None]}
        per = {k: [] for k in ("camera_normal", "camera_position", "distance", "z_depth", "ray_direction", "cos_ray_normal")}
        for b in range(a.views):
            p, n = ops.interpolate(pcam[b], rast, fd), unit(ops.interpolate(ncam[b], rast, fd))
            d = torch.sqrt((p * p).sum(-1, keepdim=True))
            rd = p / d.clamp_min(1e-12)
            per["camera_normal"].append(sel(n, -1.0)); per["camera_position"].append(p); per["distance"].append(d)
            per["z_depth"].append(p[..., 2:]); per["ray_direction"].append(sel(rd, -1.0)); per["cos_ray_normal"].append(sel((n * rd).sum(-1, keepdim=True), -1.0))
        out.update({k: torch.stack(v) for k, v in per.items()})
        return out

    x, y = fused(), composed()
    worst = max(float((x[k].float() - y[k].float()).abs().max()) for k in want)       # torch's sums have their own order: a sanity check, not a parity test
    times = {"uv_gbuffer_ms": [], "composition_ms": []}
    for it in range(a.warmup + a.iters):
        for key, fn in (("uv_gbuffer_ms", fused), ("composition_ms", composed)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[key].append(e0.elapsed_time(e1))
    bytes_out = sum(v.numel() * v.element_size() for v in x.values())
    res = {"faces": int(faces.shape[0]), "size": a.size, "views": a.views, "covered": float(cov.float().mean()), "iters": a.iters,
           "output_bytes": bytes_out, "max_abs_diff": worst}
    for k, v in times.items():
        res[k] = float(np.median(v))
        res[k.replace("_ms", "_min_ms")] = float(np.min(v))
    res["speedup"] = res["composition_ms"] / res["uv_gbuffer_ms"]
    res["uv_gbuffer_output_GBps"] = bytes_out / res["uv_gbuffer_ms"] / 1e6
    print(json.dumps(res))


if __name__ == "__main__":
    main()
