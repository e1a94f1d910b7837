#!/usr/bin/env python
"""Environment renderer: the fused kernels of csrc/scene.hip against the composition that was available before them, in one process.

    python tools/bench_scene.py [--views 6] [--size 1024] [--cube 512] [--pano 1024 2048] [--out profiles/scene_bench.log]

  render   6 x 1024^2 views from a 512^2 cubemap and a 1024 x 2048 panorama, every output (rays_d, cubemap_attr, uv, latlong_map_attr)
           composition: torch elementwise rays and uv, ops.cube_sample, a wrap-linear lookup from torch index arithmetic and gathers
  c2l      cubemap_to_latlong to 1024 x 2048;  composition: torch direction grid (fp64, rounded once) + ops.cube_sample
  bake     6 x 1024^2 views into 1024 x 2048;  composition: torch matmuls, F.grid_sample, sum / count, nan_to_num, clamp
Device time by events, medians of 30 after 5 warm-ups, the two sides interleaved; peak device memory of each side above what is allocated before it runs.
Reported, not gated."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rays_torch(c2ws, intr, H, W):
    dev = c2ws.device
    nx = ((torch.arange(W, device=dev, dtype=torch.float32) + 0.5) / W) * 2.0 - 1.0
    ny = ((torch.arange(H, device=dev, dtype=torch.float32) + 0.5) / H) * 2.0 - 1.0
    px = ((nx + (2 * intr[0, 2] - 1)) / (2 * intr[0, 0]))[None, :].expand(H, W)
    py = (((2 * intr[1, 2] - 1) - ny) / (2 * intr[1, 1]))[:, None].expand(H, W)
    p = torch.stack([px, py, -torch.ones_like(px)], -1)
    d = torch.einsum("bij,hwj->bhwi", c2ws[:, :3, :3], p)
    return torch.nn.functional.normalize(d, dim=-1)


def _wrap_linear_torch(lat, uv):
    Hi, Wi, _ = lat.shape
    x, y = uv[..., 0] * Wi - 0.5, uv[..., 1] * Hi - 0.5
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    ix0, iy0 = torch.remainder(x0.long(), Wi), torch.remainder(y0.long(), Hi)
    ix1, iy1 = torch.remainder(ix0 + 1, Wi), torch.remainder(iy0 + 1, Hi)
    top = lat[iy0, ix0] * (1 - fx) + lat[iy0, ix1] * fx
    bot = lat[iy1, ix0] * (1 - fx) + lat[iy1, ix1] * fx
    return top * (1 - fy) + bot * fy


def _texel_dirs_torch(Ht, Wt, dev):
    gx = 2.0 * ((torch.arange(Wt, device=dev, dtype=torch.float64) + 0.5) / Wt) - 1.0
    gy = 2.0 * ((torch.arange(Ht, device=dev, dtype=torch.float64) + 0.5) / Ht) - 1.0
    psi, theta = (gx * torch.pi)[None, :], (gy * (torch.pi / 2) + torch.pi / 2)[:, None]
    return torch.stack(torch.broadcast_tensors(torch.sin(theta) * torch.sin(psi), torch.cos(theta), -torch.sin(theta) * torch.cos(psi)), -1).float().contiguous()


def _measure(pairs, warmup=5, iters=30):
    """pairs: [(name, fn)] timed interleaved -> {name: (median ms, peak bytes above the baseline allocation)}"""
    for _ in range(warmup):
        for _, fn in pairs:
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in pairs}
    for _ in range(iters):
        for n, fn in pairs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b))
    out = {}
    for n, fn in pairs:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        out[n] = (sorted(times[n])[len(times[n]) // 2], torch.cuda.max_memory_allocated() - base)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--cube", type=int, default=512)
    ap.add_argument("--pano", type=int, nargs=2, default=[1024, 2048])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from unitex_amd.texturetools import camera, ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    B, S, N, (Ht, Wt) = a.views, a.size, a.cube, a.pano
    c2ws = camera.generate_orbit_views_c2ws(B, radius=0.3, height=0.1, theta_0=10.0, degree=True).float().to(dev).contiguous()
    intr = camera.generate_intrinsics(60.0, 60.0, fov=True, degree=True).float().to(dev).contiguous()
    cube = torch.rand(6, N, N, 3, generator=g).to(dev)
    lat = torch.rand(Ht, Wt, 3, generator=g).to(dev)
    images = torch.rand(B, S, S, 3, generator=g).to(dev)
    w2cs = torch.linalg.inv(c2ws.cpu()).to(dev).contiguous()
    projs = camera.intr_to_proj(intr, perspective=True).expand(B, 4, 4).contiguous()
    want = ("rays_d", "cubemap_attr", "uv", "latlong_map_attr")

    def render_torch():
        d = _rays_torch(c2ws, intr, S, S)
        ca = ops.cube_sample(cube, d.contiguous())
        uv = torch.stack([torch.atan2(d[..., 0], -d[..., 2]) / (2 * torch.pi) + 0.5, torch.acos(d[..., 1].clamp(-1, 1)) / torch.pi], -1)
        return d, ca, uv, _wrap_linear_torch(lat, uv)

    def bake_torch():
        rd = _texel_dirs_torch(Ht, Wt, dev)
        p = torch.cat([rd, torch.ones_like(rd[..., :1])], -1)
        clip = torch.matmul(torch.matmul(p, w2cs[:, None].transpose(-1, -2)), projs[:, None].transpose(-1, -2))
        depth = clip[..., 3:4]
        uv = clip[..., :2] / depth
        al = (((uv >= -1) & (uv <= 1)).all(-1, keepdim=True) & (depth > 0)).float()
        smp = torch.nn.functional.grid_sample(images.permute(0, 3, 1, 2), uv, padding_mode="zeros", align_corners=False).permute(0, 2, 3, 1)
        return ((smp * al).sum(0) / al.sum(0)).nan_to_num(nan=0.0, posinf=0.0, neginf=0.0).clamp(0.0, 1.0)

    res = {}
    res["render"] = _measure([("fused", lambda: ops.scene_render(c2ws, intr, S, S, cubemap=cube, latlong=lat, want=want)), ("composed", render_torch)])
    res["cubemap_to_latlong"] = _measure([("fused", lambda: ops.cubemap_to_latlong(cube, Ht, Wt)),
                                          ("composed", lambda: ops.cube_sample(cube, _texel_dirs_torch(Ht, Wt, dev)))])
    res["bake"] = _measure([("fused", lambda: ops.scene_bake_latlong(w2cs, projs, Ht, Wt, images)), ("composed", bake_torch)])
    # the two sides compute the same thing (loose: the composition's fp32 coordinates differ in the last bits)
    f, c = ops.scene_render(c2ws, intr, S, S, cubemap=cube, latlong=lat, want=want), render_torch()
    agree = {"render_cube": (f["cubemap_attr"] - c[1]).abs().max().item(), "render_latlong_median": (f["latlong_map_attr"] - c[3]).abs().median().item(),
             "bake_median": (ops.scene_bake_latlong(w2cs, projs, Ht, Wt, images)[2] - bake_torch()).abs().median().item()}
    lines = ["scene bench: %d x %d^2 views, cubemap %d^2, panorama %d x %d, device %s" % (B, S, N, Ht, Wt, torch.cuda.get_device_name(0))]
    for k, v in res.items():
        (tf, mf), (tc, mc) = v["fused"], v["composed"]
        lines.append("%-20s fused %8.3f ms  peak %8.1f MiB | composed %8.3f ms  peak %8.1f MiB | speed-up %5.2fx  memory %5.2fx" %
                     (k, tf, mf / 2 ** 20, tc, mc / 2 ** 20, tc / tf, mc / max(mf, 1)))
    lines.append("agreement of the two sides (max / median abs difference): " + json.dumps(agree))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
