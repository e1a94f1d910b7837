#!/usr/bin/env python
"""Time and peak device memory of the scattered-sample UV bake (reported in DESIGN.md 8, not gated): six 512^2 orbit views into a 1024^2 atlas of the ~50 k-face
sphere, NVDiffRendererInverse.global_inverse_rendering(grid_interpolate_mode='nearest', normal-angle threshold 80 degrees).  Per stage (device events around the
stage, median of --reps after --warmup; the propagation loop, which reads a counter back per step, with the wall clock): the sample pass, the nearest
stage, the k-NN search, the propagation loop with its step count; and the whole call.  Each stage runs against the same stage written as the reference
writes it, in the same process: the sample pass and the propagation loop in torch on the GPU (dr.interpolate -> ops.interpolate); the nearest stage and
the k-NN search, which the reference runs on the HOST through scipy (NearestNDInterpolator, KDTree), through scipy where it is importable, once each.

    python tools/bench_global_inverse.py [--reps 20] [--log profiles/global_inverse_bench.log]"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_uv_bake import _events, _wall, interleaved, peak_mib  # noqa: E402
from unitex_amd.texturetools import camera, meshes, ops  # noqa: E402
from unitex_amd.texturetools.renderer_inverse import DeviceMesh, NVDiffRendererInverse  # noqa: E402

RENDER, TEX, K, NRM_DEG = 512, 1024, 10, 80.0


def torch_samples(rast, faces, v_uv, v_pos_cam, v_nrm_cam, normal_deg):
    """renderer_base.py:624-654 as written, dr.interpolate -> ops.interpolate (one call per view and attribute)"""
    B, H, W = rast.shape[:3]
    cov = rast[..., 3:] > 0
    attr = torch.cat([torch.nn.functional.normalize(v_pos_cam, dim=-1), v_nrm_cam], dim=-1).contiguous()
    t2p = torch.stack([ops.interpolate(v_uv, rast[b], faces) for b in range(B)])
    cam = torch.stack([ops.interpolate(attr[b].contiguous(), rast[b], faces) for b in range(B)])
    m = cov * torch.roll(cov, 1, dims=1) * torch.roll(cov, -1, dims=1) * torch.roll(cov, 1, dims=2) * torch.roll(cov, -1, dims=2)
    m = m.logical_and(cam[..., [5]] > math.cos(math.radians(normal_deg)))
    return t2p, cam, m


def torch_propagation(samples_x, idx, d2, y, pending, n_iters_max=1000):
    """renderer_base.py:702-722 as written (the [M,k,C] gather included), on the device"""
    idx = idx.long()
    d = d2.sqrt()
    score = torch.nn.functional.normalize(d.reciprocal().nan_to_num(nan=0.0), p=1, dim=-1)
    cosn = torch.nn.functional.cosine_similarity(samples_x[idx, 3:], samples_x[:, None, 3:], dim=-1)
    w = score * cosn
    pm = pending[:, None].bool()
    ny, nm = y[idx, :], pm[idx, :]
    cur = pm.logical_and(nm.sum(dim=1) < K - 1)
    steps = 0
    for _ in range(n_iters_max):
        if cur.sum() == 0:
            break
        sel = cur[:, 0]
        inv = ~nm[sel]
        ww = w[sel, :, None]
        rgb = (inv * ww * ny[sel]).sum(dim=1) / (inv * ww).sum(dim=1)
        y = torch.masked_scatter(y, cur, rgb)
        pm = pm.logical_and(cur.logical_not())
        ny, nm = y[idx, :], pm[idx, :]
        cur = pm.logical_and(nm.sum(dim=1) < K - 1)
        steps += 1
    return y, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("global inverse rendering, %s, 6 orbit views x %d^2 into a %d^2 atlas, ~50 k faces, k = %d, median of %d (ms), peak device memory above the inputs (MiB)"
        % (torch.cuda.get_device_name(0), RENDER, TEX, K, args.reps))
    verts, faces, uvs = meshes.sphere_with_faces(50000)
    mesh = DeviceMesh(verts, faces, uvs, dev)
    r = NVDiffRendererInverse(device=dev, pbr_mesh=mesh)
    c2ws = camera.generate_orbit_views_c2ws(6, radius=2.8, height=0.5)
    intr = camera.generate_intrinsics(40.0, 40.0, fov=True, degree=True).expand(6, -1, -1)
    images = torch.rand(6, RENDER, RENDER, 4, generator=torch.Generator().manual_seed(0)).to(dev)
    call = lambda: r.global_inverse_rendering(images, c2ws, intr, RENDER, TEX, grid_interpolate_mode="nearest", normal_angle_degree_threshold=NRM_DEG, n_neighbors=K)
    out = call()
    steps = r.last["inpaint_steps"]
    M, Ns, Np = out["samples_x"].shape[0], out["samples_u"].shape[0], out["predicts_u"].shape[0]
    say("faces %d, samples %d, predicted texels %d, covered texels %d, pending %d, propagation steps %d" % (
        mesh.faces.shape[0], Ns, Np, M, int((~out["map_mask"][..., 0] & (out["map_alpha"][..., 0] > 0)).sum()), steps))
    # ---- the stages of the call, by the renderer's own event brackets
    acc = {}
    for i in range(args.warmup + args.reps):
        r.stage_events = []
        call()
        torch.cuda.synchronize()
        if i >= args.warmup:
            for name, a, b in r.stage_events:
                acc.setdefault(name, []).append(a.elapsed_time(b))
    r.stage_events = None
    med = {n: sorted(v)[len(v) // 2] for n, v in acc.items()}
    whole = interleaved([("whole call", call)], _wall, args.reps, args.warmup)["whole call"]
    say("whole call %.3f ms, peak %.1f MiB; stages (device time between the brackets; the propagation bracket contains its read-backs):" % (whole, peak_mib(call)))
    for n, v in med.items():
        say("  %-14s %9.3f ms  (%4.1f %% of the call)" % (n, v, 100.0 * v / whole))
    say("the k = 1 nearest stage through utx_knn is %.1f %% of the whole call" % (100.0 * med["nearest"] / whole))
    # ---- stage against stage
    _, c2ws_cpu, _, _, rast = r._view_raster(c2ws, intr, RENDER, True)
    v_pos_cam, v_nrm_cam = ops._camera_arrays(mesh.vertices, mesh.vertex_normals, c2ws_cpu, 6, True, True, None, None)
    fused = lambda: ops.view_samples(rast, mesh.faces, mesh.uvs_2d, v_pos_cam, v_nrm_cam, True, NRM_DEG, None)
    ref = lambda: torch_samples(rast, mesh.faces, mesh.uvs_2d, v_pos_cam, v_nrm_cam, NRM_DEG)
    say("sample masks of the two passes differ on %d of %d pixels" % (int((fused()[2].bool() != ref()[2][..., 0]).sum()), rast.numel() // 4))
    k = interleaved([("utx_view_samples (one launch)", fused), ("sample pass as the reference writes it (torch + 12 interpolate launches)", ref)], _events,
                    args.reps, args.warmup)
    mem = {"utx_view_samples (one launch)": peak_mib(fused), "sample pass as the reference writes it (torch + 12 interpolate launches)": peak_mib(ref)}
    for n, v in k.items():
        say("  %-75s %9.3f ms  %8.1f MiB" % (n, v, mem[n]))
    pos = out["samples_x"][:, :3].contiguous()
    knn = lambda: ops.knn_gather(pos, pos, K, want_index=True)
    _, idx, d2 = knn()
    say("  %-75s %9.3f ms  %8.1f MiB" % ("k-NN search, utx_knn (k = %d, M = %d)" % (K, M), interleaved([("k", knn)], _events, args.reps, args.warmup)["k"], peak_mib(knn)))
    z = lambda t: torch.cat([t, torch.zeros_like(t[:, :1])], dim=-1).contiguous()
    su, pu, sv = z(out["samples_u"]), z(out["predicts_u"]), out["samples_v"].contiguous()
    near = lambda: ops.knn_gather(su, pu, 1, src_attr=sv)
    say("  %-75s %9.3f ms  %8.1f MiB" % ("nearest stage, utx_knn (k = 1, %d samples, %d texels)" % (Ns, Np), interleaved([("n", near)], _events, args.reps, args.warmup)["n"],
                                         peak_mib(near)))
    try:
        from scipy.interpolate import NearestNDInterpolator
        from scipy.spatial import KDTree
        t = time.perf_counter()
        NearestNDInterpolator(out["samples_u"].cpu().numpy(), out["samples_v"].cpu().numpy())(out["predicts_u"].cpu().numpy())
        say("  %-75s %9.3f ms  (once)" % ("nearest stage as the reference runs it (scipy NearestNDInterpolator, host)", (time.perf_counter() - t) * 1e3))
        t = time.perf_counter()
        p = pos.cpu().numpy()
        KDTree(p, leafsize=10).query(p, k=K, workers=-1)
        say("  %-75s %9.3f ms  (once)" % ("k-NN search as the reference runs it (scipy KDTree, host, all cores)", (time.perf_counter() - t) * 1e3))
    except ImportError:
        say("  scipy is not importable: the reference's host stages (NearestNDInterpolator, KDTree) are not timed")
    y0 = torch.zeros(TEX, TEX, 4, device=dev)
    y0[out["map_mask"][..., 0]] = out["predicts_v"]
    cov = out["map_alpha"][..., 0] > 0
    y0, pend = y0[cov].contiguous(), (~out["map_mask"][..., 0])[cov].to(torch.uint8).contiguous()
    nrm = out["samples_x"][:, 3:].contiguous()
    loop = lambda: ops.knn_inpaint(idx, d2, nrm, y0, pend)
    tloop = lambda: torch_propagation(out["samples_x"], idx, d2, y0, pend)
    s_ref = tloop()[1]
    assert loop()[2] == s_ref, "the two propagation loops take different numbers of steps"
    k = interleaved([("propagation loop, utx_knn_inpaint_step (%d steps, one read-back each)" % steps, loop),
                     ("propagation loop as the reference writes it (torch, [M,k,C] gathers, %d steps)" % s_ref, tloop)], _wall, args.reps, args.warmup)
    mem = dict(zip(k, (peak_mib(loop), peak_mib(tloop))))
    for n, v in k.items():
        say("  %-75s %9.3f ms  %8.1f MiB" % (n, v, mem[n]))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
