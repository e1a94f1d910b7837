#!/usr/bin/env python
"""Generate the vertex-colour-bake fixture under tests/golden/ from the REFERENCE's own Python, through the seams of make_golden.py (imported from there,
unchanged):

    python tests/golden/make_golden_vertex_bake.py            # writes tests/golden/g20_vertex_bake.npz

  G20   project_vertex_color, remapping_vertex_color, inpainting_vertex_color, initial_map_Kd_with_v_rgb (texture/reprojection/mesh_remapping.py:273-427,
        :508-627), Mesh.laplacian (mesh/structure.py:743-774): all the reference's own.
Seams: cv2, pymeshlab, trimesh, gpytoolbox and whatever else importing mesh_remapping.py asks for are the inert stubs of make_golden.install_stubs (none of
them is called on the paths taken: visualize, use_pymeshlab and use_cv_outpainting stay False); dr.rasterize / dr.interpolate -> the build's CPU rasteriser
(oracle/geom_ref.c); dr.antialias is STUBBED to identity; mesh_remapping.NVDiffRendererBase is bound to the reference's class on the CPU (its default
device is 'cuda'); Mesh.compute_uv_mask, which names 'cuda' in its body, is replaced by the same call on the CPU.  Everything else is torch's own on the
CPU.  For reference_transform=False the reference runs a second time with mesh_remapping.apply_transform WRAPPED: the wrapper inverts each matrix with the
reference's own c2w_to_w2c and hands it to the reference's apply_transform.
Logged, not restated: F.grid_sample's inputs (the two weight-map channels and the valid NDC as the reference built them) and torch.gradient's outputs
(images_arccos_grad = sqrt(dy^2 + dx^2) of them); the inpainting's step count is the number of its torch.matmul pairs.
Scene: G19's cylinder with the plate; both camera sets of G17 with G19's tighter intrinsics (B = 3), one B = 6 perspective ring for the default weight
table; render_size 48; images [B,4,20,28] with alpha 0, 1 and between; random v_rgb; use_alpha both ways; soft and hard blending; thresholds 0.05 / 0.2 /
0.5.  Asserted: (a)-(f) of the module's conditions below.  float32 / int32 / uint8, data only."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ROOT, _make_inverse_renderer, install_stubs  # noqa: E402
from make_golden_simple_rendering import _cameras  # noqa: E402
from make_golden_uv_maps import N_VIEWS, SETS  # noqa: E402
from make_golden_uv_project import INTRINSICS, scene  # noqa: E402

sys.path.insert(0, ROOT)
from oracle import vertex_bake_ref as REFN  # noqa: E402

RENDER = 48
IMG = (20, 28)
CONF = dict(overlay_confidence=0.05, blending_confidence=0.2, inpainting_confidence=0.5)
WEIGHTS3 = [2.0, 0.2, 1.0]


def g20_vertex_bake(out):
    _make_inverse_renderer()
    dr = importlib.import_module("nvdiffrast.torch")
    dr.antialias = lambda x, *a, **k: x
    S = importlib.import_module("TextureTools.texturetools.mesh.structure")
    RB = importlib.import_module("TextureTools.texturetools.render.nvdiffrast.renderer_base")
    conv = importlib.import_module("TextureTools.texturetools.camera.conversion")
    gen = importlib.import_module("TextureTools.texturetools.camera.generator")
    MR = importlib.import_module("TextureTools.texturetools.texture.reprojection.mesh_remapping")
    MR.NVDiffRendererBase = lambda *a, **k: RB.NVDiffRendererBase(device="cpu")

    def compute_uv_mask(self, texture_size):      # Mesh.compute_uv_mask (:786-799) with 'cpu' for 'cuda'
        return RB.NVDiffRendererBase(device="cpu").simple_inverse_rendering(self, None, None, None, None, None, texture_size, enable_antialis=False)["mask"][0]
    S.Mesh.compute_uv_mask = compute_uv_mask
    apply_ref = MR.apply_transform
    apply_w2c = lambda v, ts: apply_ref(v, [conv.c2w_to_w2c(t) for t in ts])
    log = {"grid": [], "grad": []}
    gs, tg, mm = torch.nn.functional.grid_sample, torch.gradient, torch.matmul

    def grid_sample(inp, grid, **kw):
        log["grid"].append((inp.detach().numpy().copy(), grid.detach().numpy().copy(), kw.get("padding_mode")))
        return gs(inp, grid, **kw)

    def gradient(*a, **k):
        r = tg(*a, **k)
        log["grad"].append([x.numpy().copy() for x in r])
        return r
    inpaint_ref = MR.inpainting_vertex_color
    steps_log = []

    def inpainting(*a, **k):
        n = [0]

        def matmul(*x, **y):
            n[0] += 1
            return mm(*x, **y)
        torch.matmul = matmul
        try:
            r = inpaint_ref(*a, **k)
        finally:
            torch.matmul = mm
        steps_log.append(n[0] // 2)
        return r
    MR.inpainting_vertex_color = inpainting

    verts, faces, uvs, nrm = scene()
    V = verts.shape[0]
    mesh = S.Mesh(torch.from_numpy(verts), torch.from_numpy(faces).long(), torch.from_numpy(uvs), torch.from_numpy(faces).long())
    mesh._v_nrm = torch.from_numpy(nrm)
    rng = np.random.default_rng(20)
    images = rng.uniform(0.0, 1.0, (6, 4) + IMG).astype(np.float32)
    sel = rng.uniform(0.0, 1.0, (6,) + IMG)
    images[:, 3] = np.where(sel < 0.3, 0.0, np.where(sel < 0.6, 1.0, images[:, 3]))
    v_rgb = rng.uniform(0.0, 1.0, (V, 3)).astype(np.float32)
    fix = dict(verts=verts, faces=faces, uvs=uvs, v_nrm=nrm, images=images, v_rgb=v_rgb, weights3=np.asarray(WEIGHTS3, np.float32),
               conf=np.asarray([CONF["overlay_confidence"], CONF["blending_confidence"], CONF["inpainting_confidence"]], np.float32))
    t_img, t_rgb = torch.from_numpy(images), torch.from_numpy(v_rgb)
    torch.nn.functional.grid_sample, torch.gradient = grid_sample, gradient
    try:
        for tag, perspective, height, theta_0 in SETS:
            c2ws, _ = _cameras(gen, perspective, height, theta_0)
            intr = gen.generate_intrinsics(*INTRINSICS[tag][:2], fov=INTRINSICS[tag][2], degree=INTRINSICS[tag][2])
            fix["c2ws_" + tag], fix["intr_" + tag] = c2ws.numpy().astype(np.float32), intr.numpy().astype(np.float32)
            r = RB.NVDiffRendererBase(device="cpu")
            if not perspective:
                r.enable_orthogonal()
            vis = r.get_visible_vertices(mesh, c2ws, intr.expand(N_VIEWS, -1, -1), RENDER).numpy()
            fix["vis_" + tag] = vis.astype(np.uint8)
            print("G20 %s: vertices hidden in every view %d, in none %d, of %d" % (tag, (~vis.any(0)).sum(), vis.all(0).sum(), V))
            w3 = torch.tensor(WEIGHTS3)
            for mode, fn in (("ref", apply_ref), ("w2c", apply_w2c)):
                MR.apply_transform = fn
                for ua in (True, False):
                    log["grid"], log["grad"] = [], []
                    acc, wacc = MR.project_vertex_color(mesh, c2ws, intr.expand(N_VIEWS, -1, -1), t_img[:3], t_rgb.clone(), w3, use_alpha=ua, render_size=RENDER,
                                                        perspective=perspective)
                    key = "%s_%s_a%d" % (tag, mode, ua)
                    fix["acc_" + key], fix["wacc_" + key] = acc.numpy(), wacc.numpy()
                    if mode == "w2c" and ua:
                        wm = np.stack([log["grid"][2 * b + 1][0][0] for b in range(N_VIEWS)]).transpose(0, 2, 3, 1)      # [B,H,W,2]
                        dy, dx = log["grad"][0]
                        grad = np.sqrt(np.square(dy) + np.square(dx))[..., 0]
                        fix["wmap_" + tag], fix["grad_" + tag] = wm.astype(np.float32), grad.astype(np.float32)
                        ndc_valid = [log["grid"][2 * b][1][0, :, 0] for b in range(N_VIEWS)]
                # every stage of remapping_vertex_color, per mode
                kw = dict(v_rgb=None, weights=WEIGHTS3, render_size=RENDER, perspective=perspective, **CONF)
                call = lambda **k: MR.remapping_vertex_color(mesh, c2ws, intr, t_img[:3], **{**kw, "v_rgb": t_rgb.clone(), **k}).numpy()
                fix["overlay_%s_%s" % (tag, mode)] = call(use_blending=False, use_inpainting=False)
                fix["soft_%s_%s" % (tag, mode)] = call(blending_type="soft", use_inpainting=False)
                fix["hard_%s_%s" % (tag, mode)] = call(blending_type="hard", use_inpainting=False)
                steps_log.clear()
                fix["final_%s_%s" % (tag, mode)] = call(blending_type="soft")
                fix["steps_%s_%s" % (tag, mode)] = np.int32(steps_log[0])
                fix["nocolour_%s_%s" % (tag, mode)] = MR.remapping_vertex_color(mesh, c2ws, intr, t_img[:3], **{**kw, "use_inpainting": False}).numpy()
            MR.apply_transform = apply_ref
            # ---- the conditions, on the w2c run
            cov = fix["wmap_" + tag][..., 0] != 0
            alpha = fix["wmap_" + tag][..., 1]
            for b in range(N_VIEWS):      # (a)
                assert (alpha[b][cov[b]] == 0).any() and (alpha[b][cov[b]] == 1).any(), "(a) %s view %d: one alpha class only on the covered pixels" % (tag, b)
            cosn = r.simple_rendering(mesh, None, None, None, c2ws, intr.expand(N_VIEWS, -1, -1), RENDER, render_cos_ray_normal=True)["cos_ray_normal"][..., 0].numpy()
            fix["cos_ray_normal_" + tag] = cosn
            g64 = REFN.weight_maps(cosn, None, 0, np.float64)["grad"]
            edge = np.abs(g64 - float(REFN.GRAD_THR32)) <= REFN.GRAD_EDGE
            assert edge[cov].sum() <= 0.005 * cov.sum(), "(b) %s: %d of %d covered pixels near the threshold" % (tag, edge[cov].sum(), cov.sum())
            near = np.zeros(V, bool)
            rim = fails = False
            for b in range(N_VIEWS):
                g = ndc_valid[b]
                ids = np.nonzero(vis[b])[0]
                fails |= len(g) < len(ids)
                rim |= bool(((np.abs(g[:, 0]) > 1 - 1.0 / IMG[1]) | (np.abs(g[:, 1]) > 1 - 1.0 / IMG[0])).any())
                ix, iy = ((g[:, 0] + 1) * RENDER - 1) / 2, ((g[:, 1] + 1) * RENDER - 1) / 2
                for ddx in (0, 1):
                    for ddy in (0, 1):
                        x, y = np.floor(ix).astype(int) + ddx, np.floor(iy).astype(int) + ddy
                        ok = (x >= 0) & (x < RENDER) & (y >= 0) & (y < RENDER)
                        hit = ok & edge[b][np.clip(y, 0, RENDER - 1), np.clip(x, 0, RENDER - 1)]
                        # the valid list is a subset of the visible list in order; a tap on an edge pixel can only be attributed when none failed
                        if hit.any():
                            near[ids[:len(hit)][hit]] = True
            fix["near_" + tag] = near.astype(np.uint8)
            assert near.sum() <= 0.02 * vis.any(0).sum(), "(c) %s: %d vertices tap a near-threshold pixel" % (tag, near.sum())
            assert rim and fails, "(d) %s: rim %s, fails the strict NDC test %s" % (tag, rim, fails)
            for mode in ("ref", "w2c"):      # (e)
                w = fix["wacc_%s_%s_a1" % (tag, mode)]
                for thr in CONF.values():
                    assert (np.abs(w - np.float32(thr)) > 1e-6).all(), "(e) %s %s: a weight within 1e-6 of %g" % (tag, mode, thr)
            assert fix["steps_%s_w2c" % tag] >= 3, "(f) %s: the inpainting took %d steps" % (tag, fix["steps_%s_w2c" % tag])
            w = fix["wacc_%s_w2c_a1" % tag]
            for thr in CONF.values():
                assert 0 < (w > thr).sum() < V, "%s: no vertex on one side of %g" % (tag, thr)
            fix["kd_" + tag] = MR.initial_map_Kd_with_v_rgb(mesh, torch.from_numpy(fix["final_%s_w2c" % tag]), texture_size=RENDER, perspective=perspective).numpy()
            print("G20 %s: visible %s, near-threshold pixels %d / %d, vertices %d, steps %d (ref mode %d), weights > thr %s" % (
                tag, vis.sum(1).tolist(), edge[cov].sum(), cov.sum(), near.sum(), fix["steps_%s_w2c" % tag], fix["steps_%s_ref" % tag],
                [int((w > t).sum()) for t in CONF.values()]))
        # ---- B = 6, the default weight table
        c2ws6 = gen.generate_orbit_views_c2ws(6, radius=2.8, height=0.3, theta_0=10.0, degree=True)
        intr6 = gen.generate_intrinsics(*INTRINSICS["p"][:2], fov=True, degree=True)
        MR.apply_transform = apply_w2c
        fix["c2ws_6"], fix["intr_6"] = c2ws6.numpy().astype(np.float32), intr6.numpy().astype(np.float32)
        fix["final_6"] = MR.remapping_vertex_color(mesh, c2ws6, intr6, t_img, v_rgb=t_rgb.clone(), render_size=RENDER, use_inpainting=False).numpy()
    finally:
        torch.nn.functional.grid_sample, torch.gradient, torch.matmul = gs, tg, mm
        MR.apply_transform, MR.inpainting_vertex_color = apply_ref, inpaint_ref
    fix = {k: np.asarray(v) for k, v in fix.items()}
    assert all(v.dtype in (np.float32, np.int32, np.uint8) for v in fix.values()), [k for k, v in fix.items() if v.dtype not in (np.float32, np.int32, np.uint8)]
    assert all(np.isfinite(v).all() for v in fix.values() if v.dtype == np.float32)
    path = os.path.join(out, "g20_vertex_bake.npz")
    np.savez_compressed(path, **fix)
    print("G20: %d arrays, %d bytes" % (len(fix), os.path.getsize(path)))
    assert os.path.getsize(path) < 1024 * 1024


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g20_vertex_bake(out)
    print("wrote g20_vertex_bake")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
