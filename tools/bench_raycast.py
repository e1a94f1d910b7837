#!/usr/bin/env python
"""Device time of the ray queries (reported in DESIGN.md 8, not gated), on the --faces benchmark sphere.  Medians of --iters after --warmup, timed with events,
the arms of each comparison interleaved (tools/bench_uv_project.timed).  Every time is that of the op as a caller sees it (kernel, output allocation, enqueue).
  (i)   self_rt fused (utx_points_enclosed, --n-rays rays per point) against the composition the reference's code implies with this library's pieces: torch-made
        [N n_rays, 3] origins and directions (randn + normalize), intersect, reshape(...).all(-1) -- for --points points all inside (radius < 0.5) and all outside
        (radius 2 .. 3), the two extremes of the early exit; with early exit switched off as a third arm; peak device memory above the resident state per form.
  (ii)  occluded against intersect-then-compare (t < 1) for --segments segments.
  (iii) intersect with all outputs against BVH.trace (id only; the quirk-preserving walk): rays per second, tree nodes visited per ray.
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_uv_project import timed  # noqa: E402


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=50000)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--n-rays", type=int, default=32)
    ap.add_argument("--segments", type=int, default=10_000_000)
    ap.add_argument("--rays", type=int, default=4_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from unitex_amd.texturetools import meshes, ops
    verts, faces, _ = meshes.sphere_with_faces(a.faces)
    v = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(faces).astype(np.int32)).cuda()
    bvh = ops.BVH(v, f)
    g = torch.Generator(device="cuda").manual_seed(666)
    res = {"faces": int(f.shape[0]), "points": a.points, "n_rays": a.n_rays, "segments": a.segments, "rays": a.rays, "iters": a.iters, "tree_depth": bvh.depth(),
           "mesh_radius": float(v.norm(dim=1).max())}

    def unit(n):
        return torch.nn.functional.normalize(torch.randn(n, 3, device="cuda", generator=g), dim=-1)

    def composed(p):
        o = p.repeat_interleave(a.n_rays, dim=0)
        d = torch.nn.functional.normalize(torch.randn(o.shape, dtype=torch.float32, device="cuda", generator=g), dim=-1)
        return (bvh.intersect(o, d, want=("tid",))["tid"] >= 0).reshape(-1, a.n_rays).all(dim=-1)

    R = res["mesh_radius"]
    for kind, lo, hi in (("inside", 0.0, 0.5 * R), ("outside", 2.0 * R, 3.0 * R)):
        p = (unit(a.points) * (lo + (hi - lo) * torch.rand(a.points, 1, device="cuda", generator=g))).contiguous()
        fused = bvh.points_enclosed(p, a.n_rays, 666)
        r = {"fused_inner_share": float(fused.float().mean()), "composed_inner_share": float(composed(p).float().mean()),
             "early_exit_changes_nothing": bool(torch.equal(fused, bvh.points_enclosed(p, a.n_rays, 666, early_exit=False)))}
        r.update(timed({"fused_ms": lambda: bvh.points_enclosed(p, a.n_rays, 666), "fused_no_early_exit_ms": lambda: bvh.points_enclosed(p, a.n_rays, 666, early_exit=False),
                        "composed_ms": lambda: composed(p)}, a.warmup, a.iters))
        r["fused_peak_bytes"] = peak_bytes(lambda: bvh.points_enclosed(p, a.n_rays, 666))
        r["composed_peak_bytes"] = peak_bytes(lambda: composed(p))
        res["self_rt_" + kind] = r
        del p, fused
    s0 = (unit(a.segments) * (2.0 * R)).contiguous()
    s1 = ((torch.rand(a.segments, 3, device="cuda", generator=g) * 2 - 1) * (1.2 * R)).contiguous()
    blocked = bvh.occluded(s0, s1)
    r = {"blocked_share": float(blocked.float().mean()),
         "agree_share": float((blocked.bool() == (bvh.intersect(s0, s1 - s0, want=("t",))["t"] < 1)).float().mean())}
    r.update(timed({"occluded_ms": lambda: bvh.occluded(s0, s1), "intersect_then_compare_ms": lambda: bvh.intersect(s0, s1 - s0, want=("t",))["t"] < 1}, a.warmup, a.iters))
    r["nodes_per_segment"] = bvh.occluded(s0, s1, count=True)[1] / a.segments
    res["occluded"] = r
    del s0, s1, blocked
    o = (unit(a.rays) * (2.0 * R)).contiguous()
    d = ((torch.rand(a.rays, 3, device="cuda", generator=g) * 2 - 1) * (0.9 * R) - o).contiguous()
    full, nodes = bvh.intersect(o, d, count=True)
    tid_trace, nodes_trace = bvh.trace_count(o, d)
    r = {"hit_share": float((full["tid"] >= 0).float().mean()), "same_id_as_trace_share": float((full["tid"] == tid_trace).float().mean()),
         "nodes_per_ray": nodes / a.rays, "trace_nodes_per_ray": nodes_trace / a.rays}
    r.update(timed({"intersect_all_ms": lambda: bvh.intersect(o, d), "intersect_tid_ms": lambda: bvh.intersect(o, d, want=("tid",)), "trace_ms": lambda: bvh.trace(o, d)},
                   a.warmup, a.iters))
    r["intersect_rays_per_second"] = a.rays / r["intersect_all_ms"] * 1e3
    r["trace_rays_per_second"] = a.rays / r["trace_ms"] * 1e3
    res["intersect"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
