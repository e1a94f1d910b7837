#!/usr/bin/env python
"""Device time of the atlas-space view projection (reported in DESIGN.md 8, not gated), on the --faces benchmark sphere with --views box cameras of
--size^2 into a --atlas^2 atlas:
  * utx_visible_faces_rays: time and tree nodes visited per ray with the rays issued in the tree's sorted leaf order and in face order;
  * utx_uv_project (uv, uv_alpha and map_attr of a per-view --size^2 x 3 image, bilinear, background 0.5) against the two compositions a caller
    could write before it, both on the raster of the visible faces per view and one ops.interpolate per view: `ops_composition`, with
    ops.screen_gbuffer's lookup for the image and for the coverage (the one tests/test_uv_project_gpu.py proves bit-identical; checked here too),
    and `composition`, with torch's grid_sample in its place (the faster of the two) -- in the same process, interleaved (A B A B ...), timed with events after --warmup rounds; medians of --iters and their ratio.
Both sides allocate their outputs inside the timed region; the rasterisations and the face masks are shared and outside it.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fns, warmup, iters):
    times = {k: [] for k in fns}
    for it in range(warmup + iters):
        for key, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[key].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=50000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--atlas", type=int, default=2048)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from unitex_amd.texturetools import camera, meshes, ops
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    verts, faces, uvs = meshes.sphere_with_faces(a.faces)
    inv = NVDiffRendererInverse(device="cuda:0").update_from_arrays(verts, faces, uvs)
    m = inv.pbr_mesh
    fd, dev = m.faces, m.vertices.device
    c2ws = camera.generate_box_views_c2ws(radius=2.8)[:a.views].float()
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    _, _, _, ndc, rast_map = inv._view_raster(c2ws, intr, a.size, True)
    rast2d = inv._uv_raster(a.atlas, a.atlas)
    B, F = rast_map.shape[0], fd.shape[0]
    bvh, c2ws_d = m.optix, c2ws.to(dev).contiguous()
    mask, n_sorted = ops.visible_faces_rays(bvh, c2ws_d, count=True)
    mask_f, n_face = ops.visible_faces_rays(bvh, c2ws_d, face_order=True, count=True)
    assert torch.equal(mask, mask_f)
    res = {"faces": int(F), "size": a.size, "atlas": a.atlas, "views": B, "iters": a.iters, "tree_depth": bvh.depth(),
           "visible_share": float(mask.float().mean()), "nodes_per_ray_sorted": n_sorted / (B * F), "nodes_per_ray_face_order": n_face / (B * F)}
    t = timed({"rays_sorted_ms": lambda: ops.visible_faces_rays(bvh, c2ws_d), "rays_face_order_ms": lambda: ops.visible_faces_rays(bvh, c2ws_d, face_order=True)},
              a.warmup, a.iters)
    res.update(t)
    g = torch.Generator().manual_seed(0)
    img = torch.rand(B, a.size, a.size, 3, generator=g).to(dev)
    tri = rast2d[..., 3].long() - 1

    def fused():
        return ops.uv_project(rast2d, fd, mask, ndc, img, rast_map, filter="bilinear", background=0.5)

    def composed():
        vis = (tri >= 0)[None] & (mask[:, tri.clamp(min=0)] != 0)
        rast_vis = torch.cat([rast2d[None, ..., :3].expand(B, -1, -1, -1), torch.where(vis, rast2d[..., 3][None], 0.0)[..., None]], -1).contiguous()
        uv = torch.stack([torch.where(vis[b][..., None], ops.interpolate(ndc[b].contiguous(), rast_vis[b], fd), -1.0) for b in range(B)])
        gs = torch.nn.functional.grid_sample
        s = gs(img.permute(0, 3, 1, 2), uv, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        cov = gs((rast_map[..., 3:4] > 0).float().permute(0, 3, 1, 2), uv, mode="nearest", align_corners=False).permute(0, 2, 3, 1)
        alpha = vis[..., None] & (cov >= 1)
        return {"uv": uv, "uv_alpha": alpha.float(), "map_attr": torch.where(alpha, s, torch.full_like(s, 0.5))}

    verts_d = m.vertices

    def composed_ops():
        """the composition the GPU test proves bit-identical: ops.interpolate per view and ops.screen_gbuffer's lookup for the image and the coverage"""
        vis = (tri >= 0)[None] & (mask[:, tri.clamp(min=0)] != 0)
        rast_vis = torch.cat([rast2d[None, ..., :3].expand(B, -1, -1, -1), torch.where(vis, rast2d[..., 3][None], 0.0)[..., None]], -1).contiguous()
        uv = torch.stack([torch.where(vis[b][..., None], ops.interpolate(ndc[b].contiguous(), rast_vis[b], fd), -1.0) for b in range(B)])
        s, cov = [], []
        for b in range(B):
            kw = dict(v_uv=ndc[b].contiguous(), want=("map_attr",))
            s.append(ops.screen_gbuffer(rast_vis[b:b + 1], fd, verts_d, maps=(img[b],), filter="bilinear", **kw)["map_attr"][0])
            covmap = (rast_map[b, ..., 3:4] > 0).float().contiguous()
            cov.append(ops.screen_gbuffer(rast_vis[b:b + 1], fd, verts_d, maps=(covmap,), filter="nearest", **kw)["map_attr"][0] >= 1)
        alpha = vis[..., None] & torch.stack(cov)
        s = torch.stack(s)
        return {"uv": uv, "uv_alpha": alpha.float(), "map_attr": torch.where(alpha, s, torch.full_like(s, 0.5))}

    z = composed_ops()
    x = fused()
    res["bit_identical_to_ops_composition"] = all(torch.equal(x[k], z[k]) for k in x)
    del z
    x, y = fused(), composed()
    res["max_abs_diff"] = max(float((x[k] - y[k]).abs().max()) for k in x)      # torch's grid_sample has its own order: a sanity check, not a parity test
    res["uv_alpha_share"] = float(x["uv_alpha"].mean())
    res.update(timed({"uv_project_ms": fused, "composition_ms": composed, "ops_composition_ms": composed_ops}, a.warmup, a.iters))
    res["speedup"] = res["composition_ms"] / res["uv_project_ms"]
    res["speedup_over_ops_composition"] = res["ops_composition_ms"] / res["uv_project_ms"]
    bytes_out = sum(v.numel() * v.element_size() for v in x.values())
    res["uv_project_output_GBps"] = bytes_out / res["uv_project_ms"] / 1e6
    print(json.dumps(res))


if __name__ == "__main__":
    main()
