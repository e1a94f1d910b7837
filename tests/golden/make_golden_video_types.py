#!/usr/bin/env python
"""Generate the turntable video-type fixture under tests/golden/ from the REFERENCE's own Python, through the same seams as
make_golden.py (imported from there, unchanged):

    python tests/golden/make_golden_video_types.py            # writes tests/golden/g13_video_types.npz

  G13   VideoExporter.export_video (video/export_nvdiffrast_video.py:37-139) on NVDiffRendererBase.uv_rendering / simple_rendering
        (render/nvdiffrast/renderer_base.py:101-350, 822-860), called with the arguments export_orbit_video passes (:157-230: background
        'white', with_alpha, normalize for z_depth / distance, ndc for the normal / position types, chunk_size 1) for the seven
        renderable video types, on the cameras export_orbit_video builds: 4 perspective frames (fov 49.1 deg) at 64^2 and 2 orthographic
        frames (scale 0.85) at 48^2 of the orbit ring at radius 2.8.
Seams: dr.rasterize / dr.interpolate -> the build's CPU rasteriser (oracle/geom_ref.c), as in the other generators; dr.antialias is
STUBBED to return its first argument (nvdiffrast's silhouette antialiasing is not part of this build: alpha = coverage).
The mesh is a flattened torus (non-convex: parts of the ring hide others, so depth ordering matters), long in x, short in z and tilted
about z: frame 0 looks down the short axis, the side frames look down the long one and reach depths on both sides of frame 0's (lo, hi),
which is what shows that the normalisation range is the first frame's only.  Its normals are the analytic torus normals (a fifth mesh
element for the build, which otherwise computes its own).
The rgb frames go through the reference's default grid_sample(bilinear, align_corners=False) on a 16^2 random texture whose row 0 is v = 0;
the uvs keep every bilinear footprint inside the texture (see _torus).
Stored: mesh, normals, uvs, texture, cameras, the per-frame rast, the per-vertex attributes the reference handed to dr.interpolate
(camera-space normals / positions, clip w), alpha once per frame, the float frames (three channels; one for z_depth / distance, whose
three are equal) and the (lo, hi) pair.  All float32, exact."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _make_inverse_renderer, install_stubs  # noqa: E402

TYPES = ["rgb", "world_normal", "camera_normal", "world_position", "camera_position", "z_depth", "distance"]
NORMALIZE = ("z_depth", "distance")
NDC = ("world_normal", "camera_normal", "world_position", "camera_position")
TEX = 16                                              # texture side
SETS = (("p", True, 4, 64), ("o", False, 2, 48))     # (tag, perspective, n_frames, render size)


def _torus(nu=28, nv=14, R=0.62, r=0.26, stretch=(1.5, 0.8, 0.45), tilt_deg=30.0):
    u = np.arange(nu) * (2 * np.pi / nu)
    v = np.arange(nv) * (2 * np.pi / nv)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    s = np.asarray(stretch)
    p = np.stack([(R + r * np.cos(vv)) * np.cos(uu), r * np.sin(vv), (R + r * np.cos(vv)) * np.sin(uu)], -1).reshape(-1, 3) * s
    n = np.stack([np.cos(vv) * np.cos(uu), np.sin(vv), np.cos(vv) * np.sin(uu)], -1).reshape(-1, 3) / s
    c, sn = np.cos(np.deg2rad(tilt_deg)), np.sin(np.deg2rad(tilt_deg))
    rot = np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]])      # about z: the side views see the ring inclined, its far half through the hole
    p, n = p @ rot.T, n @ rot.T
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    faces = []
    for i in range(nu):
        for j in range(nv):
            faces.append([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)])
            faces.append([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])
    # texel coordinates uv * TEX - 0.5 stay inside [0, TEX - 1]: no sample reaches over the texture border, where the reference's default
    # grid_sample (zero padding) and the build's rgb path (dr.texture's wrap addressing) differ by design
    uvs = (0.5 + np.stack([uu / (2 * np.pi), vv / (2 * np.pi)], -1).reshape(-1, 2) * (TEX - 1)) / TEX
    return p.astype(np.float32), np.asarray(faces, np.int32), uvs.astype(np.float32), n.astype(np.float32)


def g13_video_types(out):
    _make_inverse_renderer()           # installs the dr stubs (rasterize / interpolate -> oracle)
    dr = importlib.import_module("nvdiffrast.torch")
    V = importlib.import_module("TextureTools.texturetools.video.export_nvdiffrast_video")
    RB = importlib.import_module("TextureTools.texturetools.render.nvdiffrast.renderer_base")
    gen = importlib.import_module("TextureTools.texturetools.camera.generator")
    dr.antialias = lambda x, *a, **k: x
    rast_fn, interp_fn = dr.rasterize, dr.interpolate
    log = {"rast": [], "attr": []}

    def rasterize(ctx, pos, tri, resolution):
        r = rast_fn(ctx, pos, tri, resolution)
        log["rast"].append(r[0][0].numpy().copy())
        return r

    def interpolate(attr, rast, tri):
        log["attr"].append(attr.detach().numpy().copy())
        return interp_fn(attr, rast, tri)
    dr.rasterize, dr.interpolate = rasterize, interpolate

    verts, faces, uvs, nrm = _torus()
    rng = np.random.default_rng(13)
    tex = rng.integers(0, 256, (TEX, TEX, 3)).astype(np.uint8)
    mesh = types.SimpleNamespace(v_pos=torch.from_numpy(verts), v_nrm=torch.from_numpy(nrm), t_pos_idx=torch.from_numpy(faces).long(),
                                 v_tex=torch.from_numpy(uvs), t_tex_idx=torch.from_numpy(faces).long())
    map_Kd = torch.from_numpy(tex.astype(np.float32) / np.float32(255.0))
    texture = types.SimpleNamespace(mesh=mesh, v_rgb=None, map_Kd=map_Kd, map_Ks=None)
    fix = dict(verts=verts, faces=faces, uvs=uvs, v_nrm=nrm, tex=tex)

    orig_to = torch.Tensor.to

    def to_cpu(self, *a, **k):         # the reference moves everything to 'cuda'
        is_cuda = lambda x: (isinstance(x, str) and x.startswith("cuda")) or (isinstance(x, torch.device) and x.type == "cuda")
        a = tuple("cpu" if is_cuda(x) else x for x in a)
        if is_cuda(k.get("device")):
            k["device"] = "cpu"
        return orig_to(self, *a, **k)
    torch.Tensor.to = to_cpu
    try:
        for tag, perspective, n_frames, size in SETS:
            renderer = RB.NVDiffRendererBase(device="cpu")
            fake_self = types.SimpleNamespace(mesh_renderer=renderer)
            c2ws = gen.generate_orbit_views_c2ws(n_frames + 1, radius=2.8, height=0.0, theta_0=0.0, degree=True)[:n_frames]
            if perspective:
                intr = gen.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
                renderer.enable_perspective()
            else:
                intr = gen.generate_intrinsics(0.85, 0.85, fov=False, degree=False)
                renderer.enable_orthogonal()
            fix["c2ws_" + tag], fix["intr_" + tag] = c2ws.numpy().astype(np.float32), intr.numpy().astype(np.float32)
            for t in TYPES:
                log["rast"], log["attr"] = [], []
                video = V.VideoExporter.export_video(fake_self, texture, None, c2ws, intr, render_size=size, key=t, background="white",
                                                     with_alpha=True, normalize=t in NORMALIZE, ndc=t in NDC, chunk_size=1).numpy()
                assert video.shape == (n_frames, size, size, 4) and len(log["rast"]) == n_frames
                rast, alpha = np.stack(log["rast"]), video[..., 3]
                if "rast_" + tag in fix:
                    assert np.array_equal(fix["rast_" + tag], rast) and np.array_equal(fix["alpha_" + tag], alpha)
                fix["rast_" + tag], fix["alpha_" + tag] = rast, alpha
                if t in NORMALIZE:
                    assert np.array_equal(video[..., 0], video[..., 1]) and np.array_equal(video[..., 0], video[..., 2])
                    fix["%s_%s" % (t, tag)] = video[..., 0].copy()
                else:
                    fix["%s_%s" % (t, tag)] = video[..., :3].copy()
                # the first dr.interpolate of each frame is the type's own buffer (the second is the UV buffer of uv_rendering)
                per = len(log["attr"]) // n_frames
                own = [log["attr"][i * per] for i in range(n_frames)]
                if t == "camera_normal":
                    fix["v_nrm_cam_" + tag] = np.concatenate(own)
                elif t == "camera_position":
                    fix["v_pos_cam_" + tag] = np.concatenate(own)
                elif t == "z_depth":
                    fix["v_clip_w_" + tag] = np.concatenate(own)[..., 0]
            # (lo, hi) of the covered pixels of frame 0, before normalisation: recovered from a second, un-normalised render
            for t in NORMALIZE:
                raw = V.VideoExporter.export_video(fake_self, texture, None, c2ws, intr, render_size=size, key=t, background=None,
                                                   with_alpha=True, normalize=False, ndc=False, chunk_size=1).numpy()
                cov = raw[..., 3] > 0
                assert cov[0].any() and not cov[0].all(), "frame 0 must cover part of the image"
                lo, hi = raw[0, ..., 0][cov[0]].min(), raw[0, ..., 0][cov[0]].max()
                fix["scale_%s_%s" % (t, tag)] = np.array([lo, hi], np.float32)
                fix["raw_%s_%s" % (t, tag)] = raw[..., 0].copy()
                later = np.concatenate([raw[i, ..., 0][cov[i]] for i in range(1, n_frames)])
                print("G13 %s %s: frame 0 covers %d of %d, (lo, hi) = (%.6f, %.6f), later frames span (%.6f, %.6f)" %
                      (tag, t, int(cov[0].sum()), cov[0].size, lo, hi, later.min(), later.max()))
                if perspective:
                    assert later.min() < lo and later.max() > hi, "a later frame must leave frame 0's range"
    finally:
        torch.Tensor.to = orig_to
        dr.rasterize, dr.interpolate = rast_fn, interp_fn
    path = os.path.join(out, "g13_video_types.npz")
    np.savez_compressed(path, **fix)
    print("G13: %d arrays, %d bytes" % (len(fix), os.path.getsize(path)))


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g13_video_types(out)
    print("wrote g13_video_types")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
