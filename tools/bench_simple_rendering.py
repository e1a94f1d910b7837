#!/usr/bin/env python
"""Device time of the screen-space buffers (reported in DESIGN.md 8, not gated): utx_screen_gbuffer, every buffer of the --views box cameras and
one --map^2 x 3 map in one launch, against what a caller had to write before it -- one ops.interpolate per view and attribute plus torch for the
normalisations, norms, dot product, background selects and grid_sample -- on the same --size^2 rasters of the --faces benchmark sphere and the
same per-view per-vertex arrays, in the same process, interleaved (A B A B ...), timed with events after --warmup rounds; medians of --iters and
their ratio.  Both sides allocate their outputs inside the timed region (the caching allocator serves them after the warm-up); the rasterisation
is shared and outside it.  Prints one JSON line."""
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
    ap.add_argument("--map", type=int, default=2048)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from unitex_amd.texturetools import camera, meshes, ops
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    verts, faces, uvs = meshes.sphere_with_faces(a.faces)
    inv = NVDiffRendererInverse(device="cuda:0").update_from_arrays(verts, faces, uvs)
    m = inv.pbr_mesh
    vd, fd, nd, uv = m.vertices, m.faces, m.vertex_normals.contiguous(), m.uvs_2d
    c2ws = camera.generate_box_views_c2ws(radius=2.8)[:a.views].float()
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    mvp, _, clip, _, rast = inv._view_raster(c2ws, intr, a.size, True)
    B = rast.shape[0]
    clip_w = clip[..., 3].contiguous()
    pcam = ops.transform_points(vd, camera.c2w_to_w2c(c2ws).to(vd.device).contiguous(), want_ndc=False)[0][..., :3].contiguous()
    ncam = ops.camera_normals(nd, c2ws.to(vd.device).contiguous())
    g = torch.Generator().manual_seed(0)
    tex = torch.rand(a.map, a.map, 3, generator=g).to(vd.device)
    attr = torch.rand(vd.shape[0], 3, generator=g).to(vd.device)
    want = tuple(ops.SCREEN_GBUFFERS)
    cov = (rast[..., 3] > 0)[..., None]

    def fused():
        return ops.screen_gbuffer(rast, fd, vd, v_nrm=nd, v_uv=uv, v_attr=attr, maps=(tex,), want=want, background=0.5, clip_w=clip_w, v_pos_cam=pcam,
                                  v_nrm_cam=ncam)

    def unit(x):
        return x / torch.sqrt((x * x).sum(-1, keepdim=True)).clamp_min(1e-12)

    def composed():
        sel = lambda x, fill: torch.where(cov, x, torch.full_like(x, fill))
        interp = lambda at: torch.stack([ops.interpolate(at[b] if at.dim() == 3 else at, rast[b], fd) for b in range(B)])
        p, n = interp(pcam), unit(interp(ncam))
        d = torch.sqrt((p * p).sum(-1, keepdim=True))
        rd = p / d.clamp_min(1e-12)
        guv = sel(interp(uv), -1.0)
        sampled = torch.nn.functional.grid_sample(tex.permute(2, 0, 1)[None].expand(B, -1, -1, -1), guv, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        return {"mask": cov[..., 0].to(torch.uint8), "alpha": cov.float(), "world_normal": sel(unit(interp(nd)), -1.0), "camera_normal": sel(n, -1.0),
                "world_position": sel(interp(vd), -1.0), "camera_position": p, "distance": d, "ray_direction": sel(rd, -1.0),
                "z_depth": interp(clip_w[..., None].contiguous()), "cos_ray_normal": sel((n * rd).sum(-1, keepdim=True), -1.0),
                "v_attr": sel(interp(attr), 0.5), "uv": guv, "map_attr": sel(sampled, 0.5)}

    x, y = fused(), composed()
    worst = max(float((x[k].float() - y[k].float()).abs().max()) for k in want)       # torch's sums have their own order: a sanity check, not a parity test
    times = {"screen_gbuffer_ms": [], "composition_ms": []}
    for it in range(a.warmup + a.iters):
        for key, fn in (("screen_gbuffer_ms", fused), ("composition_ms", composed)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[key].append(e0.elapsed_time(e1))
    bytes_out = sum(v.numel() * v.element_size() for v in x.values())
    res = {"faces": int(faces.shape[0]), "size": a.size, "map": a.map, "views": B, "covered": float(cov.float().mean()), "iters": a.iters,
           "output_bytes": bytes_out, "max_abs_diff": worst}
    for k, v in times.items():
        res[k] = float(np.median(v))
        res[k.replace("_ms", "_min_ms")] = float(np.min(v))
    res["speedup"] = res["composition_ms"] / res["screen_gbuffer_ms"]
    res["screen_gbuffer_output_GBps"] = bytes_out / res["screen_gbuffer_ms"] / 1e6
    print(json.dumps(res))


if __name__ == "__main__":
    main()
