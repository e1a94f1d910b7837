#!/usr/bin/env python
"""Perspective vs orthographic back-projection, side by side in one process: NVDiffRendererInverse.infer (method='reproject') stage times
(HIP events, renderer_inverse._stage) for perspective=False (the box views, orthographic scale 1) and perspective=True (the same views,
fov 49.1 deg), iterations interleaved, plus the LBVH nodes visited per ray of each ray model (utx_bvh_trace_count over the first view's rays)
and of a control: the orthographic rays tilted 10 degrees off the view axis.  The stage brackets are the comparison; "total (events)" also holds
whatever the GPU idled waiting for the host.
usage: python tools/bench_backproject_persp.py [--faces 50000 200000] [--view 1024] [--atlas 2048] [--iters 5]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unitex_amd.texturetools import camera, meshes, ops  # noqa: E402
from unitex_amd.texturetools.benchmarks import smooth_views  # noqa: E402
from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse  # noqa: E402


def nodes_per_ray(inv, c2ws, perspective, view=0, tilt_deg=0.0):
    """mean LBVH nodes visited by the visibility rays of one view's covered texels; tilt_deg (orthographic only): the parallel rays turned
    that far off the view axis -- a control that separates the rays' obliquity to the axis-aligned boxes from the perspective origin"""
    m, rast2d = inv.pbr_mesh, inv.last["rast2d"]
    pos = ops.interpolate(m.vertices, rast2d, m.faces)[rast2d[..., 3] > 0]
    c2w = torch.as_tensor(c2ws)[view].to(pos.device, torch.float32)
    if perspective:
        ro = c2w[:3, 3].expand_as(pos).contiguous()
        d = torch.nn.functional.normalize(pos - ro, dim=-1, eps=1e-12).contiguous()
    else:
        t = math.radians(tilt_deg)
        d0 = -c2w[:3, 2] * math.cos(t) + (c2w[:3, 0] + c2w[:3, 1]) * (math.sin(t) / math.sqrt(2.0))
        d = d0.expand_as(pos).contiguous()
        ro = (pos - 2.0 * (3.0 ** 0.5) * d).contiguous()
    _, visited = m.optix.trace_count(ro, d)
    return visited / max(1, ro.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[50000, 200000])
    ap.add_argument("--view", type=int, default=1024)
    ap.add_argument("--atlas", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    dev = "cuda:0"
    c2ws = camera.generate_box_views_c2ws(2.8)[[0, 1, 4, 2, 3, 5]]
    intr = {False: camera.generate_intrinsics(1.0, 1.0, fov=False), True: camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)}
    images = torch.from_numpy(smooth_views(6, a.view, a.view)).to(dev)
    print("device: %s" % torch.cuda.get_device_name(0))
    for nf in a.faces:
        verts, faces, uvs = meshes.sphere_with_faces(nf)
        inv = NVDiffRendererInverse(device=dev).update_from_arrays(verts, faces, uvs)
        acc = {False: {}, True: {}}
        totals = {False: [], True: []}
        seen = {}
        for it in range(a.warmup + a.iters):
            for persp in (False, True):
                inv.pbr_mesh._bvh = None          # the LBVH is rebuilt per mesh, as in benchmarks.time_backprojection
                inv.stage_events = []
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                out = inv.infer(None, c2ws=c2ws, intrinsics=intr[persp], image_attrs=images, perspective=persp, H=a.view, W=a.view,
                                H2D=a.atlas, W2D=a.atlas, filt_gradient_points=False, ray_normal_angle_threhold=100.0)
                t1.record()
                torch.cuda.synchronize()
                if it < a.warmup:
                    continue
                totals[persp].append(t0.elapsed_time(t1))
                for name, e0, e1 in inv.stage_events:
                    acc[persp].setdefault(name, []).append(e0.elapsed_time(e1))
                seen[persp] = float((inv.last["winner"] >= 0).float().mean() / out[2].float().mean())
        inv.stage_events = None
        res = {"faces": int(len(faces)), "view_px": a.view, "atlas_px": a.atlas, "iters": a.iters}
        for persp in (False, True):
            key = "perspective" if persp else "orthographic"
            inv.infer(None, c2ws=c2ws, intrinsics=intr[persp], image_attrs=images, perspective=persp, H=a.view, W=a.view,
                      H2D=a.atlas, W2D=a.atlas, filt_gradient_points=False, ray_normal_angle_threhold=100.0)
            res[key] = {"total_ms": float(np.mean(totals[persp])), "stages_ms": {k: float(np.mean(v)) for k, v in acc[persp].items()},
                        "backproject_ms_all": [round(x, 4) for x in acc[persp]["backproject"]], "seen_frac_of_covered": seen[persp],
                        "nodes_per_ray_view0": nodes_per_ray(inv, c2ws, persp)}
        res["orthographic"]["nodes_per_ray_view0_tilted_10deg"] = nodes_per_ray(inv, c2ws, False, tilt_deg=10.0)
        o, p = res["orthographic"], res["perspective"]
        res["backproject_ratio"] = p["stages_ms"]["backproject"] / o["stages_ms"]["backproject"]
        print(json.dumps(res))
        print("faces %d  atlas %d^2  views 6x%d^2" % (res["faces"], a.atlas, a.view))
        print("   %-18s %12s %12s" % ("stage", "ortho ms", "persp ms"))
        for k in o["stages_ms"]:
            print("   %-18s %12.3f %12.3f" % (k, o["stages_ms"][k], p["stages_ms"].get(k, float("nan"))))
        print("   %-18s %12.3f %12.3f" % ("stage sum", sum(o["stages_ms"].values()), sum(p["stages_ms"].values())))
        print("   %-18s %12.3f %12.3f" % ("total (events)", o["total_ms"], p["total_ms"]))
        print("   backproject persp / ortho = %.3f ; nodes per ray (view 0): ortho %.1f, persp %.1f, ortho tilted 10 deg off the axis %.1f"
              % (res["backproject_ratio"], o["nodes_per_ray_view0"], p["nodes_per_ray_view0"], o["nodes_per_ray_view0_tilted_10deg"]))
        print("   seen share of covered texels: ortho %.3f, persp %.3f" % (o["seen_frac_of_covered"], p["seen_frac_of_covered"]))


if __name__ == "__main__":
    main()
