#!/usr/bin/env python
"""Generate the antialiasing fixture under tests/golden/ from the REFERENCE's own Python, through the seams of make_golden_simple_rendering.py (its helpers
are imported from there, unchanged):

    python tests/golden/make_golden_antialias.py            # writes tests/golden/g27_antialias.npz

  G27   NVDiffRendererBase.simple_rendering(enable_antialis=True) (render/nvdiffrast/renderer_base.py:101-350, the reference's default): every buffer this
        build renders, with background None, a float and a [C] tensor.
Seams: dr.rasterize / dr.interpolate -> the build's CPU rasteriser (oracle/geom_ref.c); dr.texture is not reached (bilinear grid_sample is torch's own);
dr.antialias is BOUND TO tests/support/antialias_ref.antialias_f32, this build's float32 restatement of its own rule.  nvdiffrast is not on the machines: this
fixture pins the REFERENCE'S ORDER OF OPERATIONS around dr.antialias -- which alpha each buffer is blended with, which background, what is antialiased
before what, that distance and ray_direction come from the already antialiased camera position -- and NOT nvdiffrast's samples.
Inputs (tests/support/antialias_ref.g27_scene): the 80-face sphere of radius 0.8 plus one fin, a triangle of three border edges in front of it; two views of
48 rows x 40 columns (an H / W swap cannot pass) of the orbit rings of G17 / G18, once perspective (set 'p') and once orthographic (set 'o'); a 4-channel
vertex attribute and one 16 x 24 x 3 map, 'bilinear'.
Stored per camera set: the cameras, the rasters and the clip-space vertices the reference handed to dr.rasterize / dr.antialias, the per-vertex arrays it
handed to dr.interpolate (clip_w, v_nrm_cam, v_pos_cam), every buffer of the all-flags call without a background, and v_attr / map_attr with the float and
the [C] backgrounds.  float32 / int32, exact; data only."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _make_inverse_renderer, install_stubs  # noqa: E402
from make_golden_simple_rendering import _cameras, _renderer  # noqa: E402
from make_golden_uv_maps import SETS  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.support import antialias_ref as AA  # noqa: E402


def g27_antialias(out):
    _make_inverse_renderer()           # installs the dr stubs (rasterize / interpolate -> oracle)
    dr = importlib.import_module("nvdiffrast.torch")
    RB = importlib.import_module("TextureTools.texturetools.render.nvdiffrast.renderer_base")
    gen = importlib.import_module("TextureTools.texturetools.camera.generator")
    rast_fn, interp_fn = dr.rasterize, dr.interpolate
    log = {"rast": [], "pos": [], "attr": [], "aa": 0}

    def rasterize(ctx, pos, tri, resolution):
        r = rast_fn(ctx, pos, tri, resolution)
        log["rast"].append(r[0].numpy().copy())
        log["pos"].append(pos.detach().numpy().copy())
        return r

    def interpolate(attr, rast, tri):
        log["attr"].append(attr.detach().numpy().copy())
        return interp_fn(attr, rast, tri)

    def antialias(color, rast, pos, tri):
        log["aa"] += 1
        return torch.from_numpy(AA.antialias_f32(color.detach().numpy(), rast.numpy(), pos.detach().numpy(), tri.numpy().astype(np.int32)))
    dr.rasterize, dr.interpolate, dr.antialias = rasterize, interpolate, antialias

    verts, faces, uvs, nrm, v_attr, tex = AA.g27_scene()
    H, W = AA.G27_SCREEN
    B = AA.G27_VIEWS
    fix = dict(verts=verts, faces=faces, uvs=uvs, v_nrm=nrm, v_attr=v_attr, map_0=tex, bg_float=np.float32(AA.G27_BG_FLOAT))
    rng = np.random.default_rng(270)
    bg_vec = {c: rng.uniform(0.0, 1.0, c).astype(np.float32) for c in (3, 4)}
    fix.update(bg_vec_3=bg_vec[3], bg_vec_4=bg_vec[4])
    mesh = types.SimpleNamespace(v_pos=torch.from_numpy(verts), v_nrm=torch.from_numpy(nrm), t_pos_idx=torch.from_numpy(faces).long(),
                                 v_tex=torch.from_numpy(uvs), t_tex_idx=torch.from_numpy(faces).long())
    flags = {"render_" + k: True for k in AA.G27_GEOMETRY + ("v_attr", "uv", "map_attr")}
    try:
        for tag, perspective, height, theta_0 in SETS:
            renderer = _renderer(RB, perspective)
            c2ws, intr = _cameras(gen, perspective, height, theta_0)
            c2ws = c2ws[:B]
            intr = intr[:B] if intr.dim() == 3 else intr
            fix["c2ws_" + tag], fix["intr_" + tag] = c2ws.numpy().astype(np.float32), intr.numpy().astype(np.float32)
            call = lambda **kw: renderer.simple_rendering(mesh, torch.from_numpy(v_attr), torch.from_numpy(tex), None, c2ws, intr, (H, W), **kw)
            log.update(rast=[], pos=[], attr=[], aa=0)
            res = call(**flags)           # enable_antialis=True is the reference's default
            assert sorted(res) == sorted(("mask", "alpha") + AA.G27_GEOMETRY + ("v_attr", "uv", "map_attr")), sorted(res)
            assert len(log["rast"]) == 1 and len(log["attr"]) == 9 and log["aa"] == 12      # alpha and the eleven buffers
            a = log["attr"]
            fix["rast_" + tag], fix["clip_" + tag] = log["rast"][0], log["pos"][0]
            fix["clip_w_" + tag], fix["v_nrm_cam_" + tag], fix["v_pos_cam_" + tag] = a[0][..., 0], a[2], a[4]
            assert fix["clip_" + tag].shape == (B, verts.shape[0], 4) and np.array_equal(fix["clip_w_" + tag], fix["clip_" + tag][..., 3])
            cov = res["mask"].numpy()[..., 0]
            assert res["mask"].shape == (B, H, W, 1) and np.array_equal(cov, fix["rast_" + tag][..., 3] > 0)
            alpha = res["alpha"].numpy()
            edge = (alpha > 0) & (alpha < 1)
            assert (edge[..., 0] & cov).any() and (edge[..., 0] & ~cov).any(), "no coverage estimate on both sides of the silhouette"
            fin = fix["rast_" + tag][..., 3] == len(faces)
            assert fin.reshape(B, -1).any(1).all(), "a view does not show the fin"
            for k in ("alpha",) + AA.G27_GEOMETRY + ("v_attr", "uv", "map_attr"):
                fix["%s_%s" % (k, tag)] = res[k].numpy()
            off = call(enable_antialis=False, **flags)
            assert torch.equal(off["mask"], res["mask"]) and not torch.equal(off["alpha"], res["alpha"])
            # ---- the background forms of v_attr / map_attr (None is above)
            r = call(render_v_attr=True, render_uv=True, render_map_attr=True, background=AA.G27_BG_FLOAT)
            fix["v_attr_float_" + tag], fix["map_attr_float_" + tag] = r["v_attr"].numpy(), r["map_attr"].numpy()
            r = call(render_v_attr=True, background=torch.from_numpy(bg_vec[4]))
            fix["v_attr_vec_" + tag] = r["v_attr"].numpy()
            r = call(render_uv=True, render_map_attr=True, background=torch.from_numpy(bg_vec[3]))
            fix["map_attr_vec_" + tag] = r["map_attr"].numpy()
            # distance and ray_direction without render_camera_position come from the raw position (:243, :250, :256)
            r = call(render_distance=True, render_ray_direction=True)
            fix["distance_alone_" + tag], fix["ray_direction_alone_" + tag] = r["distance"].numpy(), r["ray_direction"].numpy()
            assert not np.array_equal(fix["distance_alone_" + tag], fix["distance_" + tag])
    finally:
        dr.rasterize, dr.interpolate = rast_fn, interp_fn
    fix = {k: (v.astype(np.int32) if v.dtype.kind in "iu" else v) for k, v in fix.items()}
    assert all(v.dtype in (np.float32, np.int32) for v in fix.values()), [k for k, v in fix.items() if v.dtype not in (np.float32, np.int32)]
    assert all(np.isfinite(v).all() for v in fix.values() if v.dtype == np.float32)
    path = os.path.join(out, "g27_antialias.npz")
    np.savez_compressed(path, **fix)
    print("G27: %d arrays, %d bytes" % (len(fix), os.path.getsize(path)))
    assert os.path.getsize(path) < 1000 * 1000


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g27_antialias(out)
    print("wrote g27_antialias")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
