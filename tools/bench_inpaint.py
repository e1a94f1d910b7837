"""Telea inpainting (ops.inpaint_telea, csrc/inpaint.hip) on one MI355X: a 2048^2 atlas with the chart mask of tools/bench_uv_bake.py's scene -- the inpainting
mask (covered texels no view weighs enough) and the outpainting mask (texels the atlas does not cover) -- at radius 1 and 3, the counter read back every 1, 4 and
16 sweeps; beside it, on the same masks in the same process, the existing ops.uv_dilation and ops.pull_push.  Median of --reps (>= 20) wall-clock runs with the
sides interleaved; a side whose single call takes more than 2 s is timed --slow-reps times and says so.  There is no OpenCV on the machine, so no CPU cv2.inpaint
time stands beside these.
    python tools/bench_inpaint.py --log profiles/inpaint_bench.log"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_uv_bake import CONF, RENDER, _wall, interleaved, peak_mib  # noqa: E402
from unitex_amd.texturetools import camera, meshes, ops, remapping_uv  # noqa: E402
from unitex_amd.texturetools.renderer_inverse import DeviceMesh, NVDiffRendererInverse  # noqa: E402

TEX = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    assert args.reps >= 20, "median of at least 20"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("Telea inpainting, %s, %d^2 atlas of a %d-face sphere, 6 orbit views x %d^2; wall-clock ms per call, median of %d, sides interleaved; no OpenCV here to compare with"
        % (torch.cuda.get_device_name(0), TEX, args.faces, RENDER, args.reps))
    verts, faces, uvs = meshes.sphere_with_faces(args.faces)
    r = NVDiffRendererInverse(device=dev, pbr_mesh=DeviceMesh(verts, faces, uvs, dev))
    c2ws = camera.generate_orbit_views_c2ws(6, radius=2.8, height=0.5)
    intr = camera.generate_intrinsics(40.0, 40.0, fov=True, degree=True).expand(6, -1, -1)
    gen = torch.Generator().manual_seed(0)
    images = torch.rand(6, 4, RENDER, RENDER, generator=gen).to(dev)
    map_Kd = torch.rand(TEX, TEX, 4, generator=gen).to(dev)
    _, st = remapping_uv.remapping_uv_texture(r, c2ws, intr, images, map_Kd=map_Kd, use_cv_inpainting=False, use_inpainting=False, use_outpainting=False,
                                              render_size=RENDER, texture_size=TEX, return_stages=True, **CONF)
    rgb = st["blended"][..., :3].contiguous()
    img = (rgb.clamp(0, 1) * 255).to(torch.uint8).contiguous()
    covered = st["map_Kd"][..., 3] > 0
    masks = [("inpainting mask", st["inpaint_mask"].contiguous()), ("outpainting mask", (~covered).to(torch.uint8).contiguous())]
    for mname, hole in masks:
        d2 = ops.inpaint_distance(hole)
        depth = float(d2[hole != 0].max().item()) ** 0.5 if int(hole.sum()) else 0.0
        say("-- %s: %d of %d texels to fill, deepest %.1f texels from a known one" % (mname, int((hole != 0).sum()), TEX * TEX, depth))
        valid = (hole == 0).to(torch.uint8).contiguous()
        sides, info = [], {}
        for eps in (1, 3):
            for k in (1, 4, 16):
                name = "inpaint_telea radius %d, read-back every %2d" % (eps, k)
                fn = (lambda e, kk: (lambda: ops.inpaint_telea(img, hole, radius=e, readback=kk)))(eps, k)
                info[name] = fn()[1]
                sides.append((name, fn))
        steps = ops.uv_dilation(rgb, valid)[1]
        sides.append(("uv_dilation loop (%d steps, read-back every step)" % steps, lambda: ops.uv_dilation(rgb, valid)))
        sides.append(("pull_push", lambda: ops.pull_push(rgb, valid)))
        slow = max(_wall(fn) for _, fn in sides) > 2000.0
        reps = args.slow_reps if slow else args.reps
        if slow:
            say("   a call takes more than 2 s on this mask: median of %d, not %d" % (reps, args.reps))
        t = interleaved(sides, _wall, reps, 0 if slow else args.warmup)
        for name, fn in sides:
            sw = info.get(name)
            say("   %-58s %10.3f ms   peak %7.1f MiB%s" % (name, t[name], peak_mib(fn), "   %5d sweeps, %7.1f us per sweep" % (sw, 1e3 * t[name] / sw) if sw else ""))
        say("   utx_inpaint_distance alone: %.3f ms" % interleaved([("d", lambda: ops.inpaint_distance(hole))], _wall, args.reps, 2)["d"])
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
