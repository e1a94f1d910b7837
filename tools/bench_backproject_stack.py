#!/usr/bin/env python
"""Cost of the 9-channel (PBR stack) bake against the 3-channel path, in one process, interleaved, with HIP events around the whole infer() enqueue
and around every stage (NVDiffRendererInverse.stage_events), tree cached:
  (a) one 9-channel infer;  (b) three 3-channel infers on the channel groups;  (c) one 3-channel infer.
(b) and (c) run the thread-per-texel (C = 3) instantiation of the post-processing kernels and are the baseline.  Prints one JSON line, the per-stage table and the ratios (a)/(b), (a)/(c), and the peak
device memory of (a) and (b).
usage: python tools/bench_backproject_stack.py [--faces 50000] [--view 1024] [--atlas 2048] [--rounds 10] [--blur lens|gaussian]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unitex_amd.texturetools import camera, meshes  # noqa: E402
from unitex_amd.texturetools.benchmarks import smooth_views  # noqa: E402
from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--faces", type=int, default=50000)
ap.add_argument("--view", type=int, default=1024)
ap.add_argument("--atlas", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--blur", default="lens", choices=["lens", "gaussian"])
a = ap.parse_args()

dev = "cuda:0"
verts, faces, uvs = meshes.sphere_with_faces(a.faces)
inv = NVDiffRendererInverse(device=dev).update_from_arrays(verts, faces, uvs)
c2ws = camera.generate_box_views_c2ws(2.8)[[0, 1, 4, 2, 3, 5]]
intr = camera.generate_intrinsics(1.0, 1.0, fov=False)
base = smooth_views(6, a.view, a.view)
img9 = torch.from_numpy(np.ascontiguousarray(np.concatenate([base, base[:, ::-1, :, ::-1], 1.0 - base[:, :, ::-1]], -1), np.float32)).to(dev)
groups = [img9[..., 3 * g:3 * g + 3].contiguous() for g in range(3)]


def infer(images):
    return inv.infer(None, c2ws=c2ws, intrinsics=intr, image_attrs=images, perspective=False, H=a.view, W=a.view, H2D=a.atlas, W2D=a.atlas,
                     filt_gradient_points=False, ray_normal_angle_threhold=100.0, reproject_method=a.blur)


ARMS = {"a_nine_channels": lambda: [infer(img9)], "b_three_rgb_bakes": lambda: [infer(g) for g in groups], "c_one_rgb_bake": lambda: [infer(groups[0])]}
total = {k: [] for k in ARMS}
stages = {k: {} for k in ARMS}
peak = {}
_ = inv.pbr_mesh.optix      # the tree is built once and cached
for r in range(a.warmup + a.rounds):
    for name, fn in ARMS.items():      # interleaved: every round runs every arm
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        inv.stage_events = []
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        if r >= a.warmup:
            total[name].append(t0.elapsed_time(t1))
            acc = {}
            for st, e0, e1 in inv.stage_events:
                acc[st] = acc.get(st, 0.0) + e0.elapsed_time(e1)
            for st, v in acc.items():
                stages[name].setdefault(st, []).append(v)
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - before)
        del out
inv.stage_events = None

med = {k: float(np.median(v)) for k, v in total.items()}
res = {"faces": int(len(faces)), "view_px": a.view, "atlas_px": a.atlas, "blur": a.blur, "rounds": a.rounds,
       "total_ms_median": med, "total_ms_min": {k: float(np.min(v)) for k, v in total.items()},
       "stages_ms_median": {k: {st: float(np.median(v)) for st, v in d.items()} for k, d in stages.items()},
       "peak_bytes_above_inputs": peak,
       "ratio_a_over_b": med["a_nine_channels"] / med["b_three_rgb_bakes"], "ratio_a_over_c": med["a_nine_channels"] / med["c_one_rgb_bake"],
       "peak_ratio_a_over_b": peak["a_nine_channels"] / max(1, peak["b_three_rgb_bakes"])}
print(json.dumps(res))
names = []
for d in res["stages_ms_median"].values():
    names += [s for s in d if s not in names]
print("%-20s %12s %12s %12s   (ms, median of %d interleaved rounds; %d faces, 6 x %d^2 -> %d^2, %s blur)" % (
    "stage", "(a) 9 ch", "(b) 3 x rgb", "(c) 1 x rgb", a.rounds, len(faces), a.view, a.atlas, a.blur))
for s in names:
    print("%-20s %12s %12s %12s" % tuple([s] + ["%.3f" % res["stages_ms_median"][k][s] if s in res["stages_ms_median"][k] else "-" for k in ARMS]))
print("%-20s %12.3f %12.3f %12.3f" % tuple(["whole infer"] + [med[k] for k in ARMS]))
print("%-20s %12.3f %12.3f %12.3f" % tuple(["whole infer, min"] + [res["total_ms_min"][k] for k in ARMS]))
print("%-20s %12.1f %12.1f %12.1f   MB above the inputs" % tuple(["peak memory"] + [peak[k] / 1e6 for k in ARMS]))
print("(a)/(b) = %.3f   (a)/(c) = %.3f   peak (a)/(b) = %.3f" % (res["ratio_a_over_b"], res["ratio_a_over_c"], res["peak_ratio_a_over_b"]))
