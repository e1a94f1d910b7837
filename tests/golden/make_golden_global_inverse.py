#!/usr/bin/env python
"""Generate the scattered-sample-bake fixture under tests/golden/ from the REFERENCE's own Python, through the seams of make_golden.py and
make_golden_uv_project.py (imported from there, unchanged):

    python tests/golden/make_golden_global_inverse.py            # writes tests/golden/g25_global_inverse.npz

  G25   NVDiffRendererBase.global_inverse_rendering (render/nvdiffrast/renderer_base.py:562-743), the reference's own, with grid_interpolate_mode='nearest'
        (scipy's NearestNDInterpolator and KDTree are the real ones).
Seams: dr.rasterize / dr.interpolate -> the build's CPU rasteriser (oracle/geom_ref.c); open3d's RaycastingScene -> the float64 brute force of
make_golden_uv_project.py (Mesh.get_visible_faces).  Everything else is torch's and scipy's own on the CPU.
Logged, not restated: the rasters (views and atlas), the face masks, and -- through torch.masked_select / torch.masked_scatter, wrapped while the reference
runs -- the sample mask it selected with and the number of propagation steps it took.  v_pos_cam / v_nrm_cam are computed with the reference's expressions
(:627-628; the position NOT yet normalised, which is the form the kernel takes).
Scene: G19's cylinder with the plate, plus two triangles A and B in front of the middle perspective camera that are hinged at ONE point P: vertex P of A and
vertex P' of B are two vertex records with the same position and normal, their UVs two different texel centres (dyadic, so both texels evaluate to P exactly).
B is small (a few texels) and lies behind A, so no view sees it: its texel at P' is filled by the propagation with P's texel in its list at distance 0 as well -- the NaN path.
3 views at 48 x 48 (ring segments of G17's two rings, 30 degrees apart: perspective -30, 0, 30; G19's intrinsics), a 64 x 64 atlas, 4-channel images k / 255.
Cases: p_ray (ray threshold 60, propagation), p_plain (no threshold, no propagation), o_nrm (orthographic, normal threshold 60, propagation), p_mask (an
image_mask, no boundary exclusion, k = 4, at most 2 steps), p_tex (texture_attr / texture_mask over a block of the atlas).
Asserted: the boundary exclusion and each threshold remove samples; no threshold quantity within 1e-5 of its cosine; unseen covered texels exist and the
propagation takes >= 2 steps; the NaN path occurs (and ends at colour 0); p_mask stops at its step cap with pending texels left.  float32 / int32 / uint8."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _make_inverse_renderer, install_stubs  # noqa: E402
from make_golden_simple_rendering import _cameras  # noqa: E402
from make_golden_uv_maps import N_VIEWS, SETS  # noqa: E402
from make_golden_uv_project import INTRINSICS, install_open3d_seam, scene  # noqa: E402

RENDER, TEX = 48, 64
T = 64.0
# the hinged pair's UVs: P and P' on the texel centres (41.5, 1.5) and (53.5, 1.5); all coordinates are multiples of 1 / 128
UV_A = np.array([[41.5, 1.5], [50.0, 1.0], [41.0, 10.0]], np.float32) / np.float32(T)
UV_B = np.array([[53.5, 1.5], [56.0, 1.0], [53.0, 4.0]], np.float32) / np.float32(T)
CASES = {
    "p_ray": dict(set="p", ray_angle_degree_threshold=60.0),
    "p_plain": dict(set="p", inpainting_occlusion=False),
    "o_nrm": dict(set="o", normal_angle_degree_threshold=60.0),
    "p_mask": dict(set="p", image_mask=True, image_mask_exclude_boundary=False, n_neighbors=4, n_iters_max=2),
    "p_tex": dict(set="p", texture=True),
}


def hinged_scene(eye):
    """scene() plus the triangles A = (P, Q, R), facing the camera at `eye`, and B = (P', Q', R') behind it, P' = P"""
    verts, faces, uvs, nrm = scene()
    d = (eye / np.linalg.norm(eye)).astype(np.float64)
    e1 = np.cross(d, [0.0, 0.0, 1.0] if abs(d[2]) < 0.9 else [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    c = 0.93 * d
    P, Q, R = c + 0.05 * e1, c - 0.05 * e1 + 0.05 * e2, c - 0.05 * e1 - 0.05 * e2
    A = np.stack([P, Q, R]).astype(np.float32)
    Bt = np.stack([P, P - 0.01 * e1 + 0.005 * e2 - 0.003 * d, P - 0.01 * e1 - 0.005 * e2 - 0.003 * d]).astype(np.float32)
    Bt[0] = A[0]
    n = verts.shape[0]
    verts = np.concatenate([verts, A, Bt])
    faces = np.concatenate([faces, np.array([[n, n + 1, n + 2], [n + 3, n + 4, n + 5]], np.int32)])
    uvs = np.concatenate([uvs, UV_A, UV_B])
    nrm = np.concatenate([nrm, np.tile(d.astype(np.float32), (6, 1))])
    return verts.astype(np.float32), faces.astype(np.int32), uvs.astype(np.float32), nrm.astype(np.float32)


def g25_global_inverse(out):
    _make_inverse_renderer()
    dr = importlib.import_module("nvdiffrast.torch")
    S = importlib.import_module("TextureTools.texturetools.mesh.structure")
    install_open3d_seam()
    RB = importlib.import_module("TextureTools.texturetools.render.nvdiffrast.renderer_base")
    gen = importlib.import_module("TextureTools.texturetools.camera.generator")
    conv = importlib.import_module("TextureTools.texturetools.camera.conversion")
    log = {}
    rast_fn, gvf, msel, mscat = dr.rasterize, S.Mesh.get_visible_faces, torch.masked_select, torch.masked_scatter

    def rasterize(ctx, pos, tri, resolution):
        r = rast_fn(ctx, pos, tri, resolution)
        log.setdefault("rast", []).append(r[0].numpy().copy())
        return r

    def get_visible_faces(self, *a, **k):
        m = gvf(self, *a, **k)
        log["faces"] = m.numpy().copy()
        return m

    def masked_select(t, m):
        log.setdefault("select", []).append(m.numpy().copy())
        return msel(t, m)

    def masked_scatter(t, m, s):
        log["scatter"] = log.get("scatter", 0) + 1
        return mscat(t, m, s)

    cams = {}
    for tag, perspective, height, theta_0 in SETS:
        c2ws, _ = _cameras(gen, perspective, height, theta_0)
        # three views 30 degrees apart instead of 90 (perspective: -30, 0, 30): the back of the cylinder -- and, in the perspective set, B behind A -- is seen by none
        c2ws = gen.generate_orbit_views_c2ws(12, radius=2.8, height=height, theta_0=theta_0 - 30.0, degree=True)[:N_VIEWS]
        intr = gen.generate_intrinsics(*INTRINSICS[tag][:2], fov=INTRINSICS[tag][2], degree=INTRINSICS[tag][2])
        cams[tag] = (perspective, c2ws, intr.expand(N_VIEWS, -1, -1))
    verts, faces, uvs, nrm = hinged_scene(cams["p"][1][1, :3, 3].numpy().astype(np.float64))
    mesh = S.Mesh(torch.from_numpy(verts), torch.from_numpy(faces).long(), torch.from_numpy(uvs), torch.from_numpy(faces).long())
    mesh._v_nrm = torch.from_numpy(nrm)
    mesh.to_open3d = lambda: (verts, faces)
    rng = np.random.default_rng(25)
    img8 = rng.integers(0, 256, (N_VIEWS, RENDER, RENDER, 4)).astype(np.uint8)
    imask = (rng.uniform(0.0, 1.0, (N_VIEWS, RENDER, RENDER, 1)) < 0.7)
    tex8 = rng.integers(0, 256, (TEX, TEX, 4)).astype(np.uint8)
    tmask = np.zeros((TEX, TEX, 1), bool)
    tmask[20:44, 8:30] = True
    images = torch.from_numpy(img8.astype(np.float32) / np.float32(255.0))
    fix = dict(verts=verts, faces=faces, uvs=uvs, v_nrm=nrm, images_u8=img8, image_mask=imask.astype(np.uint8), texture_u8=tex8,
               texture_mask=tmask.astype(np.uint8), render_size=np.int32(RENDER), texture_size=np.int32(TEX))
    dr.rasterize, S.Mesh.get_visible_faces, torch.masked_select, torch.masked_scatter = rasterize, get_visible_faces, masked_select, masked_scatter
    try:
        for name, case in CASES.items():
            case = dict(case)
            tag = case.pop("set")
            perspective, c2ws, intr = cams[tag]
            kw = dict(grid_interpolate_mode="nearest")
            if case.pop("image_mask", False):
                kw["image_mask"] = torch.from_numpy(imask)
            if case.pop("texture", False):
                kw["texture_attr"], kw["texture_mask"] = torch.from_numpy(tex8.astype(np.float32) / np.float32(255.0)), torch.from_numpy(tmask)
            kw.update(case)
            r = RB.NVDiffRendererBase(device="cpu")
            r.enable_perspective() if perspective else r.enable_orthogonal()
            log.clear()
            ret = r.global_inverse_rendering(mesh, images, c2ws, intr, RENDER, TEX, **kw)
            view = [x for x in log["rast"] if x.shape[1:3] == (RENDER, RENDER)]
            atlas = [x for x in log["rast"] if x.shape[1:3] == (TEX, TEX)]
            rast = view[-1] if view[-1].shape[0] == N_VIEWS else np.concatenate(view[-N_VIEWS:])
            if "rast_" + tag not in fix:
                v_pos_homo = torch.cat([mesh.v_pos, torch.ones_like(mesh.v_pos[..., :1])], dim=-1)
                fix["c2ws_" + tag], fix["intr_" + tag] = c2ws.numpy().astype(np.float32), intr.numpy().astype(np.float32)
                fix["rast_" + tag], fix["rast2d"] = rast.astype(np.float32), atlas[-1][0].astype(np.float32)
                fix["face_mask_" + tag] = log["faces"].astype(np.uint8)
                fix["v_pos_cam_" + tag] = torch.matmul(v_pos_homo, conv.c2w_to_w2c(c2ws).permute(0, 2, 1))[:, :, :3].numpy().astype(np.float32)
                fix["v_nrm_cam_" + tag] = torch.nn.functional.normalize(torch.matmul(mesh.v_nrm, c2ws[:, :3, :3]), dim=-1).numpy().astype(np.float32)
                fix["tex_to_pos_" + tag], fix["tex_to_pos_cam_" + tag] = ret["tex_to_pos"].numpy(), ret["tex_to_pos_cam"].numpy()
                fix["world_to_tex"] = ret["world_to_tex"].numpy()
            assert (fix["rast_" + tag] == rast).all() and (fix["face_mask_" + tag] == log["faces"]).all()
            mask = log["select"][0][..., 0]
            fix["mask_" + name] = np.packbits(mask, axis=-1)
            fix["n_samples_" + name] = np.int32(ret["samples_u"].shape[0])
            fix["map_attr_" + name] = ret["map_attr"].numpy()
            fix["map_mask_" + name] = np.packbits(ret["map_mask"].numpy()[..., 0], axis=-1)
            fix["map_alpha"] = ret["map_alpha"].numpy()[..., 0].astype(np.uint8)
            steps = 0
            if ret["samples_y"] is not None:
                y = ret["samples_y"].numpy()
                steps = log.get("scatter", 0)      # torch.masked_scatter is the loop's own (:718); the two outside it are Tensor methods
                fix["nan_" + name] = np.isnan(y).any(-1).astype(np.uint8)
            fix["steps_" + name] = np.int32(steps)
            # ---- the conditions
            cov = rast[..., 3] > 0
            cam = ret["tex_to_pos_cam"].numpy()
            dot = (cam[..., :3] * cam[..., 3:]).sum(-1)
            msg = "%s: samples %d of %d covered" % (name, mask.sum(), cov.sum())
            if kw.get("image_mask_exclude_boundary", True) and not any(k in kw for k in ("ray_angle_degree_threshold", "normal_angle_degree_threshold")):
                assert mask.sum() < cov.sum(), "%s: the boundary exclusion removed nothing" % name
            for key, q in (("ray_angle_degree_threshold", dot), ("normal_angle_degree_threshold", cam[..., 5])):
                if key in kw:
                    c = np.cos(np.radians(kw[key]))
                    assert (q[cov] > c).any() and (q[cov] <= c).any(), "%s: %s splits nothing" % (name, key)
                    assert (np.abs(q[cov] - c) > 1e-5).all(), "%s: a pixel within 1e-5 of the cosine of %s" % (name, key)
            covered = fix["map_alpha"] > 0
            unseen = covered & ~ret["map_mask"].numpy()[..., 0]
            assert unseen.any(), "%s: every covered texel is seen" % name
            if name in ("p_ray", "o_nrm"):
                assert steps >= 2, "%s: the propagation took %d steps" % (name, steps)
            if name == "p_ray":
                assert fix["nan_" + name].sum() >= 1, "p_ray: the NaN path did not occur"
                assert (fix["map_attr_" + name][covered][fix["nan_" + name] > 0] == 0).all()
            if name == "p_mask":
                assert steps == 2
            print("G25 %s, steps %d, unseen %d, NaN texels %d" % (msg, steps, unseen.sum(), fix.get("nan_" + name, np.zeros(1)).sum()))
    finally:
        dr.rasterize, S.Mesh.get_visible_faces, torch.masked_select, torch.masked_scatter = rast_fn, gvf, msel, mscat
    # the hinge: both texels evaluate to P exactly
    w2t = fix["world_to_tex"]
    assert (w2t[1, 41, :3] == verts[-6]).all() and (w2t[1, 53, :3] == verts[-6]).all(), "the hinge texels do not both evaluate to P"
    fm = fix["face_mask_p"]
    assert fm[:, -2].any() and not fm[:, -1].any(), "A must be seen by a view and B by none: %s" % fm[:, -2:].tolist()
    fix = {k: np.asarray(v) for k, v in fix.items()}
    assert all(v.dtype in (np.float32, np.int32, np.uint8) for v in fix.values()), [k for k, v in fix.items() if v.dtype not in (np.float32, np.int32, np.uint8)]
    assert all(np.isfinite(v).all() for v in fix.values() if v.dtype == np.float32)
    path = os.path.join(out, "g25_global_inverse.npz")
    np.savez_compressed(path, **fix)
    print("G25: %d arrays, %d bytes" % (len(fix), os.path.getsize(path)))
    assert os.path.getsize(path) < 640 * 1024


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g25_global_inverse(out)
    print("wrote g25_global_inverse")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
