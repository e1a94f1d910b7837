#!/usr/bin/env python
"""Generate the atlas-space geometry-buffer fixture under tests/golden/ from the REFERENCE's own Python, through the same seams as
make_golden.py (imported from there, unchanged):

    python tests/golden/make_golden_uv_maps.py            # writes tests/golden/g17_uv_maps.npz

  G17   NVDiffRendererBase.simple_inverse_rendering (render/nvdiffrast/renderer_base.py:352-489) with every flag this build renders
        (world_normal, world_position, camera_normal, camera_position, distance, z_depth, ray_direction, cos_ray_normal) in ONE call per
        camera set, and world_normal / world_position once more with c2ws=None.
Seams: dr.rasterize / dr.interpolate -> the build's CPU rasteriser (oracle/geom_ref.c), as in the other generators; dr.antialias is
STUBBED to return its first argument (nvdiffrast's silhouette antialiasing is not part of this build: alpha = coverage).
Two lines of the reference do not reach a stored value with that stub: `batch_size = c2ws.shape` (:446) rebinds batch_size to a torch.Size,
which only the voxel / uv branches (:432, :514; not requested here) read afterwards; and the z_depth branch hands t_pos_idx instead of
t_tex_idx to dr.antialias (:466), whose stub ignores it.
Inputs, small but able to go wrong:
  * a non-square atlas of 48 rows x 40 columns (render_size=(48, 40)): an H / W swap cannot pass;
  * a mesh of two UV charts (two patches of a cylinder, each with vertices of its own) separated by a gutter of background texels, so
    that the coverage mask and both background values (-1 and 0) matter;
  * vertex normals that are the analytic cylinder normals scaled by lengths between 0.5 and 2 (both normalisations matter: the per-vertex
    one in front of dr.interpolate and the per-texel one behind it), and ONE zero-length vertex normal (F.normalize's 1e-12 clamp:
    its camera-space normal is 0 / 1e-12 = 0);
  * B = 3 cameras of an orbit ring at radius 2.8, twice: set 'p' (ring at height 0 from theta 0, stored with perspective intrinsics, fov
    49.1 deg, renderer.enable_perspective()) and set 'o' (ring at height 0.7 from theta 45 deg, orthographic intrinsics, scale 0.85,
    renderer.enable_orthogonal()).  The function never projects -- only c2ws enters it, the intrinsics are stored for completeness -- so
    the two sets stand on different rings: what differs between them, and is the point, is w2c.
Stored: mesh (verts, faces int32, uvs, v_nrm), the atlas raster, mask, alpha, the world buffers of the all-flags call and of the c2ws=None
call (none_*), and per camera set the cameras, the per-vertex arrays the reference handed to dr.interpolate (v_nrm_cam, v_pos_cam) and
every camera-dependent buffer.  All float32, exact; data only."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _make_inverse_renderer, install_stubs  # noqa: E402

ATLAS = (48, 40)                                       # (H, W)
WORLD = ("world_normal", "world_position")
PER_VIEW = ("camera_normal", "camera_position", "distance", "z_depth", "ray_direction", "cos_ray_normal")
SETS = (("p", True, 0.0, 0.0), ("o", False, 0.7, 45.0))     # (tag, perspective, ring height, theta_0 in degrees)
N_VIEWS = 3


def _two_charts(nu=5, nv=6):
    """two patches of a cylinder about y (radius 0.7, squashed in z), (nu + 1) x (nv + 1) vertices each, no vertex shared"""
    verts, nrm, uvs, faces = [], [], [], []
    rng = np.random.default_rng(17)
    for chart, (a0, a1, u0, u1) in enumerate(((-1.2, 0.6, 0.06, 0.44), (1.4, 3.3, 0.57, 0.95))):
        base = len(verts)
        for i in range(nu + 1):
            for j in range(nv + 1):
                a = a0 + (a1 - a0) * i / nu
                y = -0.8 + 1.6 * j / nv
                verts.append([0.7 * np.sin(a), y, 0.45 * np.cos(a) + 0.1 * chart])
                n = np.array([np.sin(a) / 0.7, 0.15 * y, np.cos(a) / 0.45])
                nrm.append(n / np.linalg.norm(n) * rng.uniform(0.5, 2.0))
                uvs.append([u0 + (u1 - u0) * i / nu, 0.08 + 0.86 * j / nv])
        idx = lambda i, j: base + i * (nv + 1) + j
        for i in range(nu):
            for j in range(nv):
                faces.append([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)])
                faces.append([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])
    nrm = np.asarray(nrm)
    nrm[2 * (nv + 1) + 3] = 0.0                         # an interior vertex of chart 0: six triangles interpolate it
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32), np.asarray(uvs, np.float32), nrm.astype(np.float32)


def g17_uv_maps(out):
    _make_inverse_renderer()           # installs the dr stubs (rasterize / interpolate -> oracle)
    dr = importlib.import_module("nvdiffrast.torch")
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

    verts, faces, uvs, nrm = _two_charts()
    mesh = types.SimpleNamespace(v_pos=torch.from_numpy(verts), v_nrm=torch.from_numpy(nrm), t_pos_idx=torch.from_numpy(faces).long(),
                                 v_tex=torch.from_numpy(uvs), t_tex_idx=torch.from_numpy(faces).long())
    fix = dict(verts=verts, faces=faces, uvs=uvs, v_nrm=nrm)
    flags = {"render_" + k: True for k in WORLD + PER_VIEW}
    H, W = ATLAS
    try:
        for tag, perspective, height, theta_0 in SETS:
            renderer = RB.NVDiffRendererBase(device="cpu")
            c2ws = gen.generate_orbit_views_c2ws(N_VIEWS + 1, radius=2.8, height=height, theta_0=theta_0, degree=True)[:N_VIEWS]
            if perspective:
                intr = gen.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
                renderer.enable_perspective()
            else:
                intr = gen.generate_intrinsics(0.85, 0.85, fov=False, degree=False)
                renderer.enable_orthogonal()
            fix["c2ws_" + tag], fix["intr_" + tag] = c2ws.numpy().astype(np.float32), intr.numpy().astype(np.float32)
            log["rast"], log["attr"] = [], []
            res = renderer.simple_inverse_rendering(mesh, None, None, None, c2ws, intr, ATLAS, **flags)
            assert sorted(res) == sorted(("mask", "alpha") + WORLD + PER_VIEW), sorted(res)
            # dr.interpolate saw, in the order of the source: v_nrm, v_nrm_cam, v_pos, v_pos_cam and, for cos_ray_normal, the two per-view arrays again
            assert len(log["rast"]) == 1 and len(log["attr"]) == 6
            assert np.array_equal(log["attr"][0], nrm) and np.array_equal(log["attr"][2], verts)
            assert np.array_equal(log["attr"][1], log["attr"][4]) and np.array_equal(log["attr"][3], log["attr"][5])
            fix["v_nrm_cam_" + tag], fix["v_pos_cam_" + tag] = log["attr"][1], log["attr"][3]
            assert fix["v_nrm_cam_" + tag].shape == fix["v_pos_cam_" + tag].shape == (N_VIEWS, verts.shape[0], 3)
            shared = dict(rast=log["rast"][0], mask=res["mask"].numpy()[0].astype(np.float32), alpha=res["alpha"].numpy()[0])
            for k in WORLD:
                assert res[k].shape == (1, H, W, 3)
                shared[k] = res[k].numpy()
            for k, v in shared.items():       # the camera-independent part does not depend on the set
                assert k not in fix or np.array_equal(fix[k], v), k
                fix[k] = v
            for k in PER_VIEW:
                assert res[k].shape == (N_VIEWS, H, W, 1 if k in ("distance", "z_depth", "cos_ray_normal") else 3), (k, res[k].shape)
                fix["%s_%s" % (k, tag)] = res[k].numpy()
        log["rast"], log["attr"] = [], []
        res = renderer.simple_inverse_rendering(mesh, None, None, None, None, None, ATLAS, render_world_normal=True, render_world_position=True)
        assert sorted(res) == sorted(("mask", "alpha") + WORLD)
        assert np.array_equal(log["rast"][0], fix["rast"]) and np.array_equal(res["alpha"].numpy()[0], fix["alpha"])
        for k in WORLD:
            fix["none_" + k] = res[k].numpy()
    finally:
        dr.rasterize, dr.interpolate = rast_fn, interp_fn
    cov = fix["mask"][..., 0] > 0
    assert fix["rast"].shape == (H, W, 4) and np.array_equal(cov, fix["rast"][..., 3] > 0)
    gutter = ~cov[:, W // 2 - 1:W // 2 + 1]
    assert gutter.all() and cov[:, :W // 2].any() and cov[:, W // 2:].any(), "two charts with a gutter of background texels between them"
    assert all(v.dtype == np.float32 for k, v in fix.items() if k != "faces") and fix["faces"].dtype == np.int32
    path = os.path.join(out, "g17_uv_maps.npz")
    np.savez_compressed(path, **fix)
    print("G17: %d arrays, %d of %d texels covered, %d bytes" % (len(fix), int(cov.sum()), cov.size, os.path.getsize(path)))


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g17_uv_maps(out)
    print("wrote g17_uv_maps")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
