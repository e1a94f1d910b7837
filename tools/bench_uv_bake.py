#!/usr/bin/env python
"""Time and peak device memory of the blended UV texture bake (reported in DESIGN.md 8, not gated): six 1024^2 orbit views into a 2048^2 atlas of the ~50 k-
and ~200 k-face spheres.  utx_uv_bake (accumulation + epilogue, one launch) against the composition of the existing ops it replaces (ops.uv_project with the
[6,1024,1024,6] map, then the fp32 elementwise steps, the overlay and the soft blending in torch); one utx_uv_dilation_step launch; the dilation loop with
its read-backs (steps counted); the whole remapping_uv_texture call.  Same process, the two sides interleaved, median of --reps (>= 20) after --warmup.  The
launches are timed with device events; the loop and the whole call, which synchronise with the host, with the wall clock around a device synchronisation.
Peak memory: torch.cuda.max_memory_allocated over one call of each side, above what is allocated before it.

    python tools/bench_uv_bake.py [--faces 50000 200000] [--reps 20] [--log profiles/uv_bake_bench.log]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unitex_amd._lib import ptr  # noqa: E402
from unitex_amd.flux.ops import get_ctx  # noqa: E402
from unitex_amd.texturetools import camera, meshes, ops, remapping_uv  # noqa: E402
from unitex_amd.texturetools.renderer_inverse import DeviceMesh, NVDiffRendererInverse  # noqa: E402

RENDER, TEX = 1024, 2048
CONF = dict(overlay_confidence=0.2, blending_confidence=0.2, inpainting_confidence=0.2)


def composition(rast2d, faces, face_mask, ndc, images, wmap, rast, map_Kd, weights):
    m6 = torch.cat([images.permute(0, 2, 3, 1), wmap], dim=-1).contiguous()
    p = ops.uv_project(rast2d, faces, face_mask, ndc, m6, rast, filter="bilinear", background=None)
    rgb, c, e = torch.split(p["map_attr"], [4, 1, 1], dim=-1)
    a = p["uv_alpha"]
    w = weights[:, None, None, None] * c.square().square() * a * (1 - e)
    acc, wacc = ((a * rgb + (1 - a) * map_Kd) * w).sum(0), w.sum(0)
    out = torch.where(wacc > CONF["overlay_confidence"], acc / wacc, acc)
    bc = CONF["blending_confidence"]
    out = torch.where(wacc <= bc, (map_Kd * (bc - wacc) + out) / bc, out)
    return out, (wacc[..., 0] <= CONF["inpainting_confidence"]) & (rast2d[..., 3] > 0)


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


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


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
    say("uv bake, %s, 6 orbit views x %d^2 into a %d^2 atlas, median of %d (ms), peak device memory above the inputs (MiB)" % (
        torch.cuda.get_device_name(0), RENDER, TEX, args.reps))
    ctx = get_ctx(0)
    for n_faces in args.faces:
        verts, faces, uvs = meshes.sphere_with_faces(n_faces)
        mesh = DeviceMesh(verts, faces, uvs, dev)
        r = NVDiffRendererInverse(device=dev, pbr_mesh=mesh)
        c2ws = camera.generate_orbit_views_c2ws(6, radius=2.8, height=0.5)
        intr = camera.generate_intrinsics(40.0, 40.0, fov=True, degree=True).expand(6, -1, -1)
        gen = torch.Generator().manual_seed(0)
        images = torch.rand(6, 4, RENDER, RENDER, generator=gen).to(dev)
        map_Kd = torch.rand(TEX, TEX, 4, generator=gen).to(dev)
        weights = torch.tensor(remapping_uv.default_weights(6), device=dev)
        _, c2ws_cpu, _, ndc, rast = r._view_raster(c2ws, intr, RENDER, True)
        cosn = ops.screen_gbuffer(rast, mesh.faces, mesh.vertices, v_nrm=mesh.vertex_normals, c2ws=c2ws_cpu, want=["cos_ray_normal"])["cos_ray_normal"]
        wmap = ops.view_weight_maps(cosn, None, r=ops.weight_map_radius(RENDER))
        rast2d = r._uv_raster(TEX, TEX)
        face_mask = r._visible_faces(c2ws, True, "rays", None, 0)
        epi = dict(blending="soft", **CONF)
        fused = lambda: ops.uv_bake(rast2d, mesh.faces, face_mask, ndc, images, wmap, rast, map_Kd, weights, epilogue=epi)
        comp = lambda: composition(rast2d, mesh.faces, face_mask, ndc, images, wmap, rast, map_Kd, weights)
        _, _, blended, mask = fused()
        ref, ref_mask = comp()
        say("-- %d faces (%d vertices): fused and composition differ by at most %.3g on the blended atlas, masks differ on %d texels" % (
            faces.shape[0], verts.shape[0], float((blended - ref).abs().max()), int((mask.bool() != ref_mask).sum())))
        k = interleaved([("utx_uv_bake (accumulation + epilogue)", fused), ("composition: uv_project + torch", comp)], _events, args.reps, args.warmup)
        mem = {"utx_uv_bake (accumulation + epilogue)": peak_mib(fused), "composition: uv_project + torch": peak_mib(comp)}
        rgb = blended[..., :3].contiguous()
        valid = (1 - mask).contiguous()
        nxt, mnxt = torch.empty_like(rgb), torch.empty_like(valid)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        one = lambda: ctx.check(ctx.lib.utx_uv_dilation_step(ctx.handle, ptr(rgb), ptr(valid), TEX, TEX, 3, 0, ptr(nxt), ptr(mnxt), ptr(counter), ctx.stream()))
        k.update(interleaved([("utx_uv_dilation_step (one launch, no read-back)", one)], _events, args.reps, args.warmup))
        steps = ops.uv_dilation(rgb, valid)[1]
        k.update(interleaved([("uv_dilation loop with read-backs (%d steps)" % steps, lambda: ops.uv_dilation(rgb, valid))], _wall, args.reps, args.warmup))
        whole = lambda: remapping_uv.remapping_uv_texture(r, c2ws, intr, images, map_Kd=map_Kd, use_cv_inpainting=False, render_size=RENDER, texture_size=TEX)
        k.update(interleaved([("remapping_uv_texture, whole call", whole)], _wall, args.reps, args.warmup))
        for name, ms in k.items():
            say("   %-58s %9.3f%s" % (name, ms, "   peak %8.1f MiB" % mem[name] if name in mem else ""))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
