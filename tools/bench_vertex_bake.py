#!/usr/bin/env python
"""Time of the vertex-colour bake (reported in DESIGN.md 8, not gated): six 1024^2 orbit views onto the ~50 k- and ~200 k-face spheres, per kernel
(utx_view_weight_maps, utx_vertex_project_blend, the utx_vertex_inpaint_step loop) and for the whole remapping_vertex_color call, each against a
torch-on-GPU composition of the same steps written here (arccos / torch.gradient / max_pool2d, grid_sample per view, a sparse Laplacian product per step).
Same process, the two sides interleaved, median of --reps (>= 20) after --warmup.  The kernels are timed with device events; the inpainting loops and the
whole call, which synchronise with the host at every step, with the wall clock around a device synchronisation.

    python tools/bench_vertex_bake.py [--faces 50000 200000] [--reps 20] [--log profiles/vertex_bake_bench.log]"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unitex_amd.texturetools import camera, meshes, ops, remapping  # noqa: E402
from unitex_amd.texturetools.renderer_inverse import DeviceMesh, NVDiffRendererInverse  # noqa: E402

RENDER = 1024
CONF = dict(overlay_confidence=0.2, blending_confidence=0.2, inpainting_confidence=0.2)


def torch_weight_maps(cosn, r):
    c = cosn.clamp(-1.0, 0.0)
    a = ((torch.arccos(c) - torch.pi / 2) / (torch.pi / 2)).clamp(0.0, 1.0)
    dy, dx = torch.gradient(a, dim=[1, 2])
    alpha = (torch.sqrt(dy.square() + dx.square()) > math.radians(10) / (math.pi / 2)).float()
    if r > 0:
        alpha = torch.nn.functional.max_pool2d(alpha.permute(0, 3, 1, 2), 2 * r + 1, 1, r).permute(0, 2, 3, 1)
    return torch.cat([c, alpha], -1)


def torch_project_blend(v_pos, vis, xform, proj, images, wmap, v_rgb, weights):
    """the dense form of the reference's loop (masks instead of index lists), then the overlay and the soft blending"""
    homo = torch.cat([v_pos, torch.ones_like(v_pos[:, :1])], -1)
    acc, wacc = torch.zeros_like(v_rgb), torch.zeros_like(v_rgb[:, :1])
    for b in range(vis.shape[0]):
        clip = (homo @ xform[b].T) @ proj[b].T
        ndc = clip[:, :2] / clip[:, 3:]
        ok = vis[b] & torch.logical_and(ndc > -1, ndc < 1).all(-1)
        g = ndc.nan_to_num(0.0).clamp(-2, 2)[None, :, None]
        rgba = torch.nn.functional.grid_sample(images[b][None], g, padding_mode="reflection", mode="bilinear", align_corners=False)[0, :, :, 0].T
        cw = torch.nn.functional.grid_sample(wmap[b][None].permute(0, 3, 1, 2), g, padding_mode="zeros", mode="bilinear", align_corners=False)[0, :, :, 0].T
        a = rgba[:, 3:]
        c = rgba[:, :3] * a + v_rgb * (1 - a)
        w = torch.where(ok[:, None], weights[b] * cw[:, :1].square().square() * (1 - cw[:, 1:]), torch.zeros_like(a))
        acc = acc + w * torch.where(ok[:, None], c, v_rgb)
        wacc = wacc + w
    out = torch.where(wacc > CONF["overlay_confidence"], acc / wacc, acc)
    bc = CONF["blending_confidence"]
    out = torch.where(wacc <= bc, (v_rgb * (bc - wacc) + out) / bc, out)
    return out, wacc


def torch_inpaint(L, v_rgb, idx, max_iters=1000):
    v_rgb = v_rgb.clone()
    v_mask = torch.ones_like(v_rgb[:, :1])
    v_mask[idx] = 0
    cnt, steps = v_mask.sum(), 0
    L_inv = torch.index_select(L, 0, idx)
    for _ in range(max_iters):
        m_rgb, m_mask = torch.matmul(L_inv, v_rgb * v_mask), torch.matmul(L_inv, v_mask)
        v_rgb[idx] = torch.where(m_mask > 0, m_rgb / m_mask, v_rgb[idx])
        v_mask[idx] = (m_mask > 0).float()
        steps += 1
        cur = v_mask.sum()
        if cur > cnt:      # the reference's comparison: one host synchronisation per step here as well
            cnt = cur
        else:
            break
    return v_rgb, steps


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def interleaved(pairs, timer, reps, warmup):
    """pairs: [(name, fn)]; every repetition runs each of them once, in order -> {name: median ms}"""
    for _ in range(warmup):
        for _, fn in pairs:
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in pairs}
    for _ in range(reps):
        for n, fn in pairs:
            times[n].append(timer(fn))
    return {n: statistics.median(v) for n, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[50000, 200000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    assert args.reps >= 20, "median of at least 20"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("vertex bake, %s, 6 orbit views x %d^2, images 6 x 4 x 1024 x 1024, median of %d (ms)" % (torch.cuda.get_device_name(0), RENDER, args.reps))
    for n_faces in args.faces:
        verts, faces, uvs = meshes.sphere_with_faces(n_faces)
        mesh = DeviceMesh(verts, faces, uvs, dev)
        r = NVDiffRendererInverse(device=dev, pbr_mesh=mesh)
        V = verts.shape[0]
        c2ws = camera.generate_orbit_views_c2ws(6, radius=2.8, height=0.5)
        intr = camera.generate_intrinsics(40.0, 40.0, fov=True, degree=True).expand(6, -1, -1)
        gen = torch.Generator().manual_seed(0)
        images = torch.rand(6, 4, 1024, 1024, generator=gen).to(dev)
        v_rgb = torch.rand(V, 3, generator=gen).to(dev)
        weights = torch.tensor(remapping.default_weights(6), device=dev)
        vis = r.get_visible_vertices(c2ws, perspective=True, method="raster", intrinsics=intr, render_size=RENDER)
        cosn = r.simple_rendering(c2ws, intr, RENDER, perspective=True, render_cos_ray_normal=True)["cos_ray_normal"]
        rad = ops.weight_map_radius(RENDER)
        wmap = ops.view_weight_maps(cosn, r=rad)
        xform = camera.c2w_to_w2c(c2ws).to(dev).contiguous()
        proj = camera.intr_to_proj(intr, perspective=True).to(dev).contiguous()
        vis8 = vis.to(torch.uint8).contiguous()
        epi = dict(blending="soft", **CONF)
        _, wacc, blended, mask = ops.vertex_project(mesh.vertices, vis8, xform, proj, images, wmap, v_rgb, weights, epilogue=epi)
        idx = torch.nonzero(mask)[:, 0]
        rowptr, col = ops.vertex_adjacency(mesh.faces, V)
        deg = (rowptr[1:] - rowptr[:-1]).float()
        row = torch.repeat_interleave(torch.arange(V, device=dev), (rowptr[1:] - rowptr[:-1]).long())
        L = torch.sparse_coo_tensor(torch.stack([row, col.long()]), deg[row], (V, V)).coalesce()
        steps = ops.vertex_inpaint(rowptr, col, blended, idx)[1]
        t_steps = torch_inpaint(L, blended, idx)[1]
        t_out, t_wacc = torch_project_blend(mesh.vertices, vis, xform, proj, images, wmap, v_rgb, weights)
        say("-- %d faces, %d vertices, dilation radius %d, %d vertices to inpaint, %d steps (torch: %d); max |blended - torch| %.3g" % (
            faces.shape[0], V, rad, idx.numel(), steps, t_steps, float((blended - t_out).abs().max())))
        k = interleaved([("utx_view_weight_maps", lambda: ops.view_weight_maps(cosn, r=rad)), ("torch weight maps", lambda: torch_weight_maps(cosn, rad)),
                         ("utx_vertex_project_blend", lambda: ops.vertex_project(mesh.vertices, vis8, xform, proj, images, wmap, v_rgb, weights, epilogue=epi)),
                         ("torch projection + blend", lambda: torch_project_blend(mesh.vertices, vis, xform, proj, images, wmap, v_rgb, weights))],
                        _events, args.reps, args.warmup)
        one = ops.vertex_inpaint      # a single step without the read-back: max_iters = 1 still reads once; the launch alone is timed through the C ABI
        from unitex_amd._lib import ptr
        from unitex_amd.flux.ops import get_ctx
        ctx = get_ctx(0)
        m8 = torch.ones(V, dtype=torch.uint8, device=dev)
        m8[idx] = 0
        nxt, m8n, cnt, idx32 = blended.clone(), m8.clone(), torch.zeros(1, dtype=torch.int32, device=dev), idx.to(torch.int32).contiguous()
        step = lambda: ctx.check(ctx.lib.utx_vertex_inpaint_step(ctx.handle, ptr(rowptr), ptr(col), ptr(idx32), idx32.numel(), ptr(blended), ptr(m8), ptr(nxt),
                                                                 ptr(m8n), ptr(cnt), ctx.stream()))
        if idx32.numel():
            k.update(interleaved([("utx_vertex_inpaint_step (one launch, no read-back)", step)], _events, args.reps, args.warmup))
        w = interleaved([("vertex_inpaint (%d steps, one read-back each)" % steps, lambda: one(rowptr, col, blended, idx)),
                         ("torch inpainting (%d steps)" % t_steps, lambda: torch_inpaint(L, blended, idx)),
                         ("remapping_vertex_color (whole call)", lambda: remapping.remapping_vertex_color(r, c2ws, intr, images, v_rgb, render_size=RENDER))],
                        _wall, args.reps, args.warmup)
        for name, ms in list(k.items()) + list(w.items()):
            say("   %-58s %9.3f" % (name, ms))
        if idx32.numel():
            launch = k["utx_vertex_inpaint_step (one launch, no read-back)"]
            loop = w["vertex_inpaint (%d steps, one read-back each)" % steps]
            say("   inpainting: %d launches x %.3f ms = %.3f ms of device work in a loop of %.3f ms: the per-step read-back and host work take %.0f %%" % (
                steps, launch, steps * launch, loop, 100.0 * (1.0 - steps * launch / loop)))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
