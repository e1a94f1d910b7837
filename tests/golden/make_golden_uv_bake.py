#!/usr/bin/env python
"""Generate the blended-UV-bake fixture under tests/golden/ from the REFERENCE's own Python, through the seams of make_golden.py, make_golden_uv_project.py
and make_golden_vertex_bake.py (imported from there, unchanged):

    python tests/golden/make_golden_uv_bake.py            # writes tests/golden/g21_uv_bake.npz

  G21   project_uv_texture, remapping_uv_texture (texture/reprojection/mesh_remapping.py:145-270, :430-505), uv_dilation
        (texture/reprojection/uv_dilation.py:33-50, :80-92) and pull_push: all the reference's own.
Seams: cv2, pymeshlab, trimesh and whatever else importing mesh_remapping.py asks for are the inert stubs of make_golden.install_stubs (none is called:
visualize, use_cv_inpainting and use_cv_outpainting stay False); dr.rasterize / dr.interpolate -> the build's CPU rasteriser (oracle/geom_ref.c);
dr.antialias is STUBBED to identity; open3d's RaycastingScene -> the float64 brute force of make_golden_uv_project.py (Mesh.get_visible_faces);
mesh_remapping.NVDiffRendererBase is bound to the reference's class on the CPU; Mesh.compute_uv_mask, which names 'cuda' in its body, is replaced by the
same call on the CPU.  Everything else is torch's own on the CPU.
Logged, not restated: what the reference's simple_inverse_rendering returned inside project_uv_texture (uv_alpha; the coverage lookup is the nearest
grid_sample it makes), the map it sampled (the two weight channels), the rasters (atlas and views), v_ndc = the attribute it interpolated, the face masks;
uv_dilation's inputs, output and step count (the number of _uv_dilation_v2 calls).
Scene: G19 / G20's cylinder with the plate; both camera sets of G17 with G19's tighter intrinsics (B = 3), one B = 6 perspective ring for the default weight
table; render_size 48, images 48 x 48 (k / 255, stored as uint8) with alpha 0, 1 and between; texture_size 64; a 4-channel map_Kd (k / 255); use_alpha both
ways; soft and hard blending; thresholds 0.05 / 0.2 / 0.5.
Readings recorded: (a) map_Kd=None raises RuntimeError in the reference (stored as text); (b) and (c) are what the stored arrays show: the accumulators follow
uv_alpha, not the image's alpha, and with use_alpha=False the texels off a view's coverage carry texel [0, 0] of its six channels.
Asserted: texels seen by 0, 1 and >= 2 views; accumulated weights on both sides of each confidence and none within 1e-6 of one; both edge-alpha classes
sampled; an inpainting region at least 2 dilation steps deep.  Whether a texel with vis but without coverage occurs is PRINTED, not asserted
(tests/test_uv_bake_gpu.py makes one by hand).  float32 / int32 / uint8 / text, data only."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ROOT, _make_inverse_renderer, install_stubs  # noqa: E402
from make_golden_simple_rendering import _cameras  # noqa: E402
from make_golden_uv_maps import N_VIEWS, SETS  # noqa: E402
from make_golden_uv_project import INTRINSICS, install_open3d_seam, scene  # noqa: E402

RENDER, TEX = 48, 64
CONF = dict(overlay_confidence=0.05, blending_confidence=0.2, inpainting_confidence=0.5)
WEIGHTS3 = [2.0, 0.3, 1.0]      # not 0.2: with use_alpha=False a texel off every coverage would weigh exactly a confidence


def g21_uv_bake(out):
    _make_inverse_renderer()
    dr = importlib.import_module("nvdiffrast.torch")
    dr.antialias = lambda x, *a, **k: x
    S = importlib.import_module("TextureTools.texturetools.mesh.structure")
    install_open3d_seam()      # after structure.py is imported: its annotations want the stub's classes
    RB = importlib.import_module("TextureTools.texturetools.render.nvdiffrast.renderer_base")
    gen = importlib.import_module("TextureTools.texturetools.camera.generator")
    MR = importlib.import_module("TextureTools.texturetools.texture.reprojection.mesh_remapping")
    UD = importlib.import_module("TextureTools.texturetools.texture.reprojection.uv_dilation")
    log = {}

    class Renderer(RB.NVDiffRendererBase):
        def __init__(self, *a, **k):
            super().__init__(device="cpu")

        def simple_inverse_rendering(self, mesh, v_attr, map_attr, *a, **k):
            ret = super().simple_inverse_rendering(mesh, v_attr, map_attr, *a, **k)
            if k.get("render_map_attr"):
                log["inv"] = {n: ret[n].detach().numpy().copy() for n in ("uv", "uv_alpha", "map_attr")}
                log["map"] = map_attr.detach().numpy().copy()
            return ret
    MR.NVDiffRendererBase = Renderer

    def compute_uv_mask(self, texture_size):      # Mesh.compute_uv_mask (:786-799) with 'cpu' for 'cuda'
        return RB.NVDiffRendererBase(device="cpu").simple_inverse_rendering(self, None, None, None, None, None, texture_size, enable_antialis=False)["mask"][0]
    S.Mesh.compute_uv_mask = compute_uv_mask
    rast_fn, interp_fn, gvf = dr.rasterize, dr.interpolate, S.Mesh.get_visible_faces

    def rasterize(ctx, pos, tri, resolution):
        r = rast_fn(ctx, pos, tri, resolution)
        log.setdefault("rast", []).append(r[0].numpy().copy())
        return r

    def interpolate(attr, rast, tri):
        log.setdefault("attr", []).append(attr.detach().numpy().copy())
        return interp_fn(attr, rast, tri)

    def get_visible_faces(self, *a, **k):
        m = gvf(self, *a, **k)
        log["faces"] = m.numpy().copy()
        return m
    step_ref, dil_ref = UD._uv_dilation_v2, MR.uv_dilation

    def step(*a, **k):
        log["steps"] = log.get("steps", 0) + 1
        return step_ref(*a, **k)

    def dilation(kd, mask, *a, **k):
        log["steps"] = 0
        log["dil_in"], log["dil_mask"] = kd.detach().numpy().copy(), mask.detach().numpy().copy()
        r = dil_ref(kd, mask, *a, **k)
        log["dil_out"] = r.detach().numpy().copy()
        return r

    verts, faces, uvs, nrm = scene()
    mesh = S.Mesh(torch.from_numpy(verts), torch.from_numpy(faces).long(), torch.from_numpy(uvs), torch.from_numpy(faces).long())
    mesh._v_nrm = torch.from_numpy(nrm)
    mesh.to_open3d = lambda: (verts, faces)
    rng = np.random.default_rng(21)
    img8 = rng.integers(0, 256, (6, 4, RENDER, RENDER)).astype(np.uint8)
    sel = rng.uniform(0.0, 1.0, (6, RENDER, RENDER))
    img8[:, 3] = np.where(sel < 0.3, 0, np.where(sel < 0.6, 255, img8[:, 3]))
    kd8 = rng.integers(0, 256, (TEX, TEX, 4)).astype(np.uint8)
    images, map_Kd = img8.astype(np.float32) / np.float32(255.0), kd8.astype(np.float32) / np.float32(255.0)
    fix = dict(verts=verts, faces=faces, uvs=uvs, v_nrm=nrm, images_u8=img8, map_Kd_u8=kd8, weights3=np.asarray(WEIGHTS3, np.float32),
               conf=np.asarray(list(CONF.values()), np.float32), render_size=np.int32(RENDER), texture_size=np.int32(TEX))
    t_img, t_kd = torch.from_numpy(images), torch.from_numpy(map_Kd)
    dr.rasterize, dr.interpolate, S.Mesh.get_visible_faces, UD._uv_dilation_v2, MR.uv_dilation = rasterize, interpolate, get_visible_faces, step, dilation
    try:
        def project(tag, c2ws, intr, imgs, w, perspective, ua):
            log.pop("rast", None), log.pop("attr", None)
            acc, wacc = MR.project_uv_texture(mesh, c2ws, intr.expand(c2ws.shape[0], -1, -1), imgs, t_kd.clone(), torch.as_tensor(w), use_alpha=ua, render_size=RENDER,
                                              texture_size=TEX, perspective=perspective)
            return acc.numpy(), wacc.numpy()

        def per_view_inputs(tag, B):
            """what the reference handed its own lookups in the last project_uv_texture call"""
            rasts = [r for r in log["rast"]]
            view = [r for r in rasts if r.shape[1:3] == (RENDER, RENDER)]
            atlas = [r for r in rasts if r.shape[1:3] == (TEX, TEX)]
            fix["rast2d"] = atlas[-1][0].astype(np.float32)
            fix["cover_" + tag] = (np.concatenate(view[-B:])[..., 3] > 0).astype(np.uint8) if view[-1].shape[0] == 1 else (view[-1][..., 3] > 0).astype(np.uint8)
            ndc = [a for a in log["attr"] if a.ndim == 3 and a.shape[0] == B and a.shape[-1] == 2]
            fix["v_ndc_" + tag] = ndc[-1].astype(np.float32)
            fix["face_mask_" + tag] = log["faces"].astype(np.uint8)
            fix["wmap_" + tag] = log["map"][..., 4:6].astype(np.float32)
            fix["uv_alpha_" + tag] = log["inv"]["uv_alpha"][..., 0].astype(np.uint8)
            assert fix["cover_" + tag].shape == (B, RENDER, RENDER) and fix["face_mask_" + tag].shape == (B, faces.shape[0])
            assert (log["map"][..., :4] == np.transpose(images[:B], (0, 2, 3, 1))).all()

        for tag, perspective, height, theta_0 in SETS:
            c2ws, _ = _cameras(gen, perspective, height, theta_0)
            intr = gen.generate_intrinsics(*INTRINSICS[tag][:2], fov=INTRINSICS[tag][2], degree=INTRINSICS[tag][2])
            fix["c2ws_" + tag], fix["intr_" + tag] = c2ws.numpy().astype(np.float32), intr.numpy().astype(np.float32)
            for ua in (True, False):
                fix["acc_%s_a%d" % (tag, ua)], fix["wacc_%s_a%d" % (tag, ua)] = project(tag, c2ws, intr, t_img[:3], WEIGHTS3, perspective, ua)
            project(tag, c2ws, intr, t_img[:3], WEIGHTS3, perspective, True)
            per_view_inputs(tag, N_VIEWS)
            kw = dict(weights=WEIGHTS3, render_size=RENDER, texture_size=TEX, perspective=perspective, use_cv_inpainting=False, **CONF)
            call = lambda **k: MR.remapping_uv_texture(mesh, c2ws, intr.expand(N_VIEWS, -1, -1), t_img[:3], **{**kw, "map_Kd": t_kd.clone(), **k}).numpy()
            for blending in ("soft", "hard"):
                fix["blended_%s_%s" % (blending, tag)] = call(blending_type=blending, use_inpainting=False, use_outpainting=False)[..., :3]
                if blending == "hard":      # the stages after the blending do not depend on its kind: stored for 'soft' only, to keep the file small
                    continue
                fix["final_%s_%s" % (blending, tag)] = call(blending_type=blending)
                fix["steps_%s_%s" % (blending, tag)] = np.int32(log["steps"])
                fix["inpainted_%s_%s" % (blending, tag)] = np.transpose(log["dil_out"][0], (1, 2, 0)).astype(np.float32)
                fix["inpaint_mask_" + tag] = log["dil_mask"][0, 0].astype(np.uint8)
            # ---- the conditions
            ua, w = fix["uv_alpha_" + tag], fix["wacc_%s_a1" % tag][..., 0]
            covered = fix["rast2d"][..., 3] > 0
            n = ua.sum(0)
            assert (n[covered] == 0).any() and (n == 1).any() and (n >= 2).any(), "%s: texels seen by 0 / 1 / >= 2 views" % tag
            for thr in CONF.values():
                assert 0 < (w[covered] > thr).sum() < covered.sum(), "%s: no covered texel on one side of %g" % (tag, thr)
                for a in (0, 1):
                    assert (np.abs(fix["wacc_%s_a%d" % (tag, a)] - np.float32(thr)) > 1e-6).all(), "%s: a weight within 1e-6 of %g" % (tag, thr)
            e = log["inv"]["map_attr"][..., 5][ua > 0]
            assert (e == 0).any() and (e > 0).any(), "%s: one edge-alpha class only on the seen texels" % tag
            assert fix["steps_soft_" + tag] >= 2, "%s: the inpainting took %d steps" % (tag, fix["steps_soft_" + tag])
            tri = fix["rast2d"][..., 3].astype(np.int64) - 1
            vis = (tri >= 0)[None] & fix["face_mask_" + tag].astype(bool)[:, np.clip(tri, 0, None)]
            print("G21 %s: texels by views seen %s, vis without coverage %d, weights > thr %s, dilation steps %d, inpaint texels %d" % (
                tag, np.bincount(n[covered].ravel(), minlength=4).tolist(), int((vis & (ua == 0)).sum()), [int((w[covered] > t).sum()) for t in CONF.values()],
                fix["steps_soft_" + tag], int(fix["inpaint_mask_" + tag].sum())))
        # ---- B = 6, the default weight table
        c2ws6 = gen.generate_orbit_views_c2ws(6, radius=2.8, height=0.3, theta_0=10.0, degree=True)
        intr6 = gen.generate_intrinsics(*INTRINSICS["p"][:2], fov=True, degree=True)
        fix["c2ws_6"], fix["intr_6"] = c2ws6.numpy().astype(np.float32), intr6.numpy().astype(np.float32)
        fix["final_6"] = MR.remapping_uv_texture(mesh, c2ws6, intr6.expand(6, -1, -1), t_img, map_Kd=t_kd.clone(), use_cv_inpainting=False, use_inpainting=False,
                                                 use_outpainting=False, render_size=RENDER, texture_size=TEX).numpy()
        fix["acc_6"], fix["wacc_6"] = project("6", c2ws6, intr6, t_img, [2.0, 0.05, 0.2, 1.0, 0.2, 0.05], True, True)
        per_view_inputs("6", 6)
        for thr in (0.2,):
            assert (np.abs(fix["wacc_6"] - np.float32(thr)) > 1e-6).all()
        # ---- reading (a)
        try:
            MR.remapping_uv_texture(mesh, c2ws6, intr6.expand(6, -1, -1), t_img, map_Kd=None, use_cv_inpainting=False, render_size=RENDER, texture_size=TEX)
            fix["map_kd_none"] = "ran"
        except Exception as ex:      # noqa: BLE001 -- whatever the reference does is the record
            fix["map_kd_none"] = "%s: %s" % (type(ex).__name__, str(ex).splitlines()[0][:160])
        assert fix["map_kd_none"].startswith("RuntimeError"), fix["map_kd_none"]
        print("G21 map_Kd=None:", fix["map_kd_none"])
    finally:
        dr.rasterize, dr.interpolate, S.Mesh.get_visible_faces, UD._uv_dilation_v2, MR.uv_dilation = rast_fn, interp_fn, gvf, step_ref, dil_ref
    fix = {k: np.asarray(v) for k, v in fix.items()}
    assert all(v.dtype in (np.float32, np.int32, np.uint8) or v.dtype.kind == "U" for v in fix.values()), [k for k, v in fix.items() if v.dtype.kind not in "fiuU"]
    assert all(np.isfinite(v).all() for v in fix.values() if v.dtype == np.float32)
    path = os.path.join(out, "g21_uv_bake.npz")
    np.savez_compressed(path, **fix)
    print("G21: %d arrays, %d bytes" % (len(fix), os.path.getsize(path)))
    assert os.path.getsize(path) < 1024 * 1024


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g21_uv_bake(out)
    print("wrote g21_uv_bake")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
