#!/usr/bin/env python
"""Device time of silhouette antialiasing (reported in DESIGN.md 8, not gated): utx_antialias_analyze on the --views box cameras' --size^2 rasters of the
--faces benchmark sphere, utx_antialias_apply at C = 1, 3 and 9 on those weights, and simple_rendering with every geometry buffer, uv, a 3-channel v_attr and
a --map^2 x 3 map with antialias off and on, in the same process, interleaved (A B A B ...), timed with events after --warmup rounds; medians and minima of
--iters, and the achieved bytes per second of the two kernels (analysis: 16 B read + 16 B written per pixel; stencil: 16 B of weights + 8 C B per pixel).
The operator timings pre-allocate nothing: outputs come from the caching allocator inside the timed region.  Prints one JSON line."""
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
    c2ws = camera.generate_box_views_c2ws(radius=2.8)[:a.views].float()
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    _, _, clip, _, rast = inv._view_raster(c2ws, intr, a.size, True)
    B = rast.shape[0]
    opp = m.edge_opposites
    g = torch.Generator().manual_seed(0)
    tex = torch.rand(a.map, a.map, 3, generator=g).to(m.device)
    attr = torch.rand(m.vertices.shape[0], 3, generator=g).to(m.device)
    weights = ops.antialias_weights(rast, clip, m.faces, opp)
    colors = {C: torch.rand(B, a.size, a.size, C, generator=g).to(m.device) for C in (1, 3, 9)}
    flags = {"render_" + k: True for k in inv._SCREEN_FLAGS}
    render = lambda aa: inv.simple_rendering(c2ws, intr, a.size, v_attr=attr, map_attr=tex, background=0.5, antialias=aa, **flags)
    arms = [("analyze_ms", lambda: ops.antialias_weights(rast, clip, m.faces, opp))]
    arms += [("apply_c%d_ms" % C, (lambda C: lambda: ops.antialias_apply(colors[C], weights))(C)) for C in (1, 3, 9)]
    arms += [("simple_rendering_off_ms", lambda: render(False)), ("simple_rendering_on_ms", lambda: render(True))]
    times = {k: [] for k, _ in arms}
    for it in range(a.warmup + a.iters):
        for key, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[key].append(e0.elapsed_time(e1))
    npix = B * a.size * a.size
    res = {"faces": int(faces.shape[0]), "size": a.size, "views": B, "iters": a.iters, "covered": float((rast[..., 3] > 0).float().mean()),
           "pixels_with_a_weight": float((weights != 0).any(-1).float().mean())}
    for k, v in times.items():
        res[k] = float(np.median(v))
        res[k.replace("_ms", "_min_ms")] = float(np.min(v))
    res["analyze_GBps"] = 32.0 * npix / res["analyze_ms"] / 1e6
    for C in (1, 3, 9):
        res["apply_c%d_GBps" % C] = (16.0 + 8.0 * C) * npix / res["apply_c%d_ms" % C] / 1e6
    print(json.dumps(res))


if __name__ == "__main__":
    main()
