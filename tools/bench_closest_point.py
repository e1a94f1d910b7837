#!/usr/bin/env python
"""Device time of the nearest-surface query (reported in DESIGN.md 8, not gated), on the --faces benchmark sphere with --points query points of two kinds:
the points of sample_spatial (the unit cube) and those of sample_near_surface at --depth.  Per kind:
  * utx_bvh_closest_point's tree walk: milliseconds (median of --iters after --warmup, timed with events) and tree nodes visited per query, with the greedy
    first descent and without it (flags & 2);
  * the exhaustive loop of the same kernel (flags & 1) -- the cost baseline -- at the first --brute-points points: few enough to finish in seconds, enough
    to fill the machine (262 144 = 1024 workgroups), and the walk at the SAME points beside it.  Nothing is extrapolated: the two are compared at that count;
  * that walk, exhaustive loop and seedless walk return equal results on those points.
Also the time of the whole sample_spatial / sample_near_surface calls (tree given).  Every time is that of the op as a caller sees it -- the kernel plus the
allocation of its four outputs and the enqueue from Python -- which weighs on the short walks, not on the exhaustive loop.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_uv_project import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=50000)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--brute-points", type=int, default=262144)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from unitex_amd.texturetools import meshes, ops, sampling
    verts, faces, _ = meshes.sphere_with_faces(a.faces)
    v = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(faces).astype(np.int64)).cuda()
    bvh = ops.BVH(v, f.to(torch.int32).contiguous())
    N, nb = a.points, min(a.brute_points, a.points)
    res = {"faces": int(f.shape[0]), "points": N, "brute_points": nb, "depth": a.depth, "iters": a.iters, "tree_depth": bvh.depth(), "tree_nodes": 2 * int(f.shape[0]) - 1}
    kinds = {"spatial": lambda: sampling.sample_spatial(v, f, bvh=bvh, N=N, seed=666),
             "near_surface": lambda: sampling.sample_near_surface(v, f, bvh=bvh, N=N, seed=666, depth=a.depth)}
    for kind, make in kinds.items():
        pts = make()[0].contiguous()
        head = pts[:nb].contiguous()
        walk, n_seed = ops.closest_point(bvh, pts, count=True)
        _, n_plain = ops.closest_point(bvh, pts, count=True, seed_descent=False)
        w, b, s = ops.closest_point(bvh, head), ops.closest_point(bvh, head, brute=True), ops.closest_point(bvh, head, seed_descent=False)
        r = {"equal_results": all(torch.equal(w[k], b[k]) and torch.equal(w[k], s[k]) for k in w), "mean_dist": float(walk["dist"].mean()),
             "nodes_per_query": n_seed / N, "nodes_per_query_no_seed": n_plain / N}
        r.update(timed({"walk_ms": lambda: ops.closest_point(bvh, pts), "walk_no_seed_ms": lambda: ops.closest_point(bvh, pts, seed_descent=False),
                        "sampler_ms": make}, a.warmup, a.iters))
        r.update(timed({"exhaustive_ms": lambda: ops.closest_point(bvh, head, brute=True), "walk_at_brute_points_ms": lambda: ops.closest_point(bvh, head)},
                       1, 3))
        r["speedup_over_exhaustive_at_brute_points"] = r["exhaustive_ms"] / r["walk_at_brute_points_ms"]
        r["queries_per_second"] = N / r["walk_ms"] * 1e3
        res[kind] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
