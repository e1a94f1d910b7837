#!/usr/bin/env python
"""Generate the screen-space buffer fixture under tests/golden/ from the REFERENCE's own Python, through the same seams as make_golden.py
(imported from there, unchanged):

    python tests/golden/make_golden_simple_rendering.py            # writes tests/golden/g18_simple_rendering.npz

  G18   NVDiffRendererBase.simple_rendering (render/nvdiffrast/renderer_base.py:101-350): every buffer this build renders in ONE call per camera
        set (and once more with enable_antialis=False, which must equal it), map_attr per map and as a tuple in the three filter modes, v_attr
        with 1, 4 and 7 channels, every background form; and simple_inverse_rendering(render_v_attr=True) on the atlas of G17.
Seams: dr.rasterize / dr.interpolate -> the build's CPU rasteriser (oracle/geom_ref.c); dr.antialias is STUBBED to return its first argument
(alpha = coverage); dr.texture -> the restatement of nvdiffrast's linear lookup with the wrap boundary that G67n uses
(make_golden_reproject_variants.nvdiffrast_texture_linear_wrap); F.grid_sample is torch's own.
Inputs, small but able to go wrong:
  * a screen of 40 rows x 56 columns: an H / W swap cannot pass;
  * B = 3 cameras of an orbit ring at radius 2.8, twice, as in G17: set 'p' (perspective, fov 49.1 deg, height 0, theta_0 0) and set 'o'
    (orthographic, scale 0.85, height 0.7, theta_0 45 deg);
  * the two-chart cylinder of G17 with its scaled vertex normals and its one zero-length normal; its UVs rescaled so that the charts reach u, v = 0
    and 1 exactly, and then nudged on two triangles (picked as the most visible one of each chart): the three vertices of one get u = v = 0.125
    (uv = -0.75), so the pixels inside it whose interpolation returns -0.75 exactly sample column 2.5 of the 24-wide map and row / column 0.5 of the
    8 x 8 one -- exact halves below an even index, where 'nearest' rounds DOWN to even and rounding half up would pick the next texel -- and the
    three vertices of the other get u = 1, so its pixels sample column Wt - 0.5: the right tap of 'bilinear' and the tap of 'nearest' fall outside the map (zero
    padding) and 'nvdiffrast' wraps to column 0.  Both conditions are asserted below, per mode, map and camera set;
  * maps of 16 x 24 x 3 and 8 x 8 x 5 (values rounded to half precision), v_attr of 7 channels (its first 1 and 4 are the narrower ones).
The readings of the issue about the flags that stay unbuilt are CHECKED by making the calls: the type names of the exceptions are stored
(refusal_*).  Stored per camera set: cameras, the rasters, the per-vertex arrays the reference handed to dr.interpolate (clip_w, v_nrm_cam,
v_pos_cam) and every buffer.  float32 / int32 / text, exact; data only."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _make_inverse_renderer, install_stubs  # noqa: E402
from make_golden_reproject_variants import nvdiffrast_texture_linear_wrap  # noqa: E402
from make_golden_uv_maps import ATLAS, N_VIEWS, SETS, _two_charts  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.pixel_ref import grid_unnormalize  # noqa: E402

SCREEN = (40, 56)                                      # (H, W)
MODES = ("bilinear", "nearest", "nvdiffrast")
GEOMETRY = ("z_depth", "world_normal", "camera_normal", "world_position", "camera_position", "distance", "ray_direction", "cos_ray_normal")
MAP_SHAPES = ((16, 24, 3), (8, 8, 5))
BG_FLOAT = 0.25


def conditions(uv, cov, Ht, Wt):
    """per filter mode, the covered pixels with a tap outside the map, and the covered 'nearest' pixels on an exact half"""
    ix, iy = grid_unnormalize(uv[..., 0], Wt), grid_unnormalize(uv[..., 1], Ht)
    x0, y0 = np.floor(ix), np.floor(iy)
    out = {"bilinear": cov & ((x0 < 0) | (x0 + 1 >= Wt) | (y0 < 0) | (y0 + 1 >= Ht))}
    nx, ny = np.rint(ix), np.rint(iy)
    out["nearest"] = cov & ((nx < 0) | (nx >= Wt) | (ny < 0) | (ny >= Ht))
    su, sv = uv[..., 0] * np.float32(0.5) + np.float32(0.5), uv[..., 1] * np.float32(0.5) + np.float32(0.5)
    su, sv = (su - np.floor(su)) * np.float32(Wt) - np.float32(0.5), (sv - np.floor(sv)) * np.float32(Ht) - np.float32(0.5)
    out["nvdiffrast"] = cov & ((np.floor(su) < 0) | (np.floor(su) + 1 >= Wt) | (np.floor(sv) < 0) | (np.floor(sv) + 1 >= Ht))
    half = cov & (((ix - x0 == 0.5) & (x0 % 2 == 0) & (x0 + 1 < Wt)) | ((iy - y0 == 0.5) & (y0 % 2 == 0) & (y0 + 1 < Ht)))      # rint goes down, half-up goes up
    return out, half


def _cameras(gen, perspective, height, theta_0):
    c2ws = gen.generate_orbit_views_c2ws(N_VIEWS + 1, radius=2.8, height=height, theta_0=theta_0, degree=True)[:N_VIEWS]
    if perspective:
        return c2ws, gen.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    return c2ws, gen.generate_intrinsics(0.85, 0.85, fov=False, degree=False)


def _renderer(RB, perspective):
    r = RB.NVDiffRendererBase(device="cpu")
    r.enable_perspective() if perspective else r.enable_orthogonal()
    return r


def g18_simple_rendering(out):
    _make_inverse_renderer()           # installs the dr stubs (rasterize / interpolate -> oracle)
    dr = importlib.import_module("nvdiffrast.torch")
    RB = importlib.import_module("TextureTools.texturetools.render.nvdiffrast.renderer_base")
    gen = importlib.import_module("TextureTools.texturetools.camera.generator")
    dr.antialias = lambda x, *a, **k: x
    dr.texture = nvdiffrast_texture_linear_wrap
    rast_fn, interp_fn = dr.rasterize, dr.interpolate
    log = {"rast": [], "attr": []}

    def rasterize(ctx, pos, tri, resolution):
        r = rast_fn(ctx, pos, tri, resolution)
        log["rast"].append(r[0].numpy().copy())
        return r

    def interpolate(attr, rast, tri):
        log["attr"].append(attr.detach().numpy().copy())
        return interp_fn(attr, rast, tri)
    dr.rasterize, dr.interpolate = rasterize, interpolate

    verts, faces, uvs, nrm = _two_charts()
    # the charts reach 0 and 1 exactly
    lo, hi = uvs.astype(np.float64).min(0), uvs.astype(np.float64).max(0)
    at_lo, at_hi = uvs == uvs.min(0), uvs == uvs.max(0)
    uvs = ((uvs.astype(np.float64) - lo) / (hi - lo)).astype(np.float32)
    uvs[at_lo], uvs[at_hi] = 0.0, 1.0
    H, W = SCREEN
    fix = dict(verts=verts, faces=faces, v_nrm=nrm)
    rng = np.random.default_rng(18)
    maps = [rng.uniform(0.0, 1.0, s).astype(np.float16).astype(np.float32) for s in MAP_SHAPES]
    v_attr7 = rng.uniform(-1.0, 1.0, (verts.shape[0], 7)).astype(np.float32)
    fix.update(map_0=maps[0], map_1=maps[1], v_attr=v_attr7)
    tmaps = [torch.from_numpy(m) for m in maps]
    to_mesh = lambda uv: types.SimpleNamespace(v_pos=torch.from_numpy(verts), v_nrm=torch.from_numpy(nrm), t_pos_idx=torch.from_numpy(faces).long(),
                                               v_tex=torch.from_numpy(uv), t_tex_idx=torch.from_numpy(faces).long())
    try:
        # which triangles the cameras see most of: one per chart is nudged
        count = np.zeros(faces.shape[0], np.int64)
        for tag, perspective, height, theta_0 in SETS:
            c2ws, intr = _cameras(gen, perspective, height, theta_0)
            res = _renderer(RB, perspective).simple_rendering(to_mesh(uvs), None, None, None, c2ws, intr, SCREEN, enable_antialis=False)
            tid = log["rast"][-1][..., 3].astype(np.int64)
            per_view = np.stack([np.bincount(t[t > 0] - 1, minlength=faces.shape[0]) for t in tid])
            count += per_view.sum(0)
            assert res["mask"].shape == (N_VIEWS, H, W, 1)
        half_f = faces.shape[0] // 2
        f_half, f_edge = int(np.argmax(count[:half_f])), half_f + int(np.argmax(count[half_f:]))
        assert count[f_half] > 20 and count[f_edge] > 20, (count[f_half], count[f_edge])
        uvs[faces[f_half]] = 0.125
        uvs[faces[f_edge], 0] = 1.0
        fix["uvs"] = uvs
        fix["nudged_faces"] = np.array([f_half, f_edge], np.int32)
        assert uvs.min() == 0.0 and uvs.max() == 1.0 and (uvs.min(0) == 0).all() and (uvs.max(0) == 1).all()
        mesh = to_mesh(uvs)
        flags = {"render_" + k: True for k in GEOMETRY + ("v_attr", "uv", "map_attr")}
        bg_vec = {c: torch.from_numpy(rng.uniform(0.0, 1.0, c).astype(np.float32)) for c in (3, 7)}
        bb, yy, xx, cc = np.meshgrid(np.arange(N_VIEWS), np.arange(H), np.arange(W), np.arange(5), indexing="ij")
        dense = (((5 * bb + 3 * yy + xx + 7 * cc) % 16) / 16.0).astype(np.float32)      # differs between neighbours in every direction, and compresses
        bg_dense = {c: torch.from_numpy(dense[..., :c].copy()) for c in (4, 5)}
        fix.update(bg_vec_3=bg_vec[3].numpy(), bg_vec_7=bg_vec[7].numpy(), bg_dense_4=bg_dense[4].numpy(), bg_dense_5=bg_dense[5].numpy(),
                   bg_float=np.float32(BG_FLOAT))
        for tag, perspective, height, theta_0 in SETS:
            renderer = _renderer(RB, perspective)
            c2ws, intr = _cameras(gen, perspective, height, theta_0)
            fix["c2ws_" + tag], fix["intr_" + tag] = c2ws.numpy().astype(np.float32), intr.numpy().astype(np.float32)
            call = lambda **kw: renderer.simple_rendering(mesh, kw.pop("v_attr", None), kw.pop("map_attr", None), None, c2ws, intr, SCREEN, **kw)
            # ---- every buffer at once (v_attr of 4 channels, both maps as a tuple, bilinear, no background)
            log["rast"], log["attr"] = [], []
            res = call(v_attr=torch.from_numpy(v_attr7[:, :4].copy()), map_attr=tuple(tmaps), **flags)
            assert sorted(res) == sorted(("mask", "alpha") + GEOMETRY + ("v_attr", "uv", "map_attr")), sorted(res)
            # dr.interpolate saw, in the order of the source: clip w, v_nrm, v_nrm_cam, v_pos, v_pos_cam, (cos_ray_normal:) v_nrm_cam, v_pos_cam, v_attr, uv
            assert len(log["rast"]) == 1 and len(log["attr"]) == 9
            a = log["attr"]
            assert np.array_equal(a[1], nrm) and np.array_equal(a[3], verts) and np.array_equal(a[2], a[5]) and np.array_equal(a[4], a[6])
            assert np.array_equal(a[7], v_attr7[:, :4]) and np.array_equal(a[8], uvs * np.float32(2.0) - np.float32(1.0))
            fix["rast_" + tag], fix["clip_w_" + tag], fix["v_nrm_cam_" + tag], fix["v_pos_cam_" + tag] = log["rast"][0], a[0][..., 0], a[2], a[4]
            assert fix["clip_w_" + tag].shape == (N_VIEWS, verts.shape[0]) and fix["v_pos_cam_" + tag].shape == (N_VIEWS, verts.shape[0], 3)
            cov = res["mask"].numpy()[..., 0]
            assert np.array_equal(cov, fix["rast_" + tag][..., 3] > 0) and np.array_equal(res["alpha"].numpy(), res["mask"].numpy().astype(np.float32))
            assert cov.reshape(N_VIEWS, -1).any(1).all() and not cov.all()
            for k in GEOMETRY + ("uv",):
                assert res[k].shape == (N_VIEWS, H, W, {"uv": 2}.get(k, 1 if k in ("z_depth", "distance", "cos_ray_normal") else 3)), (k, res[k].shape)
                fix["%s_%s" % (k, tag)] = res[k].numpy()
            fix["v_attr4_" + tag] = res["v_attr"].numpy()
            again = call(v_attr=torch.from_numpy(v_attr7[:, :4].copy()), map_attr=tuple(tmaps), enable_antialis=False, **flags)
            for k in res:
                assert torch.equal(res[k], again[k]), "enable_antialis changes %s" % k
            # the same position buffers without render_camera_position: distance from the unmasked position
            alone = call(render_distance=True)
            assert torch.equal(alone["distance"], res["distance"])
            # ---- map_attr: each map alone and the tuple, in the three modes; the tuple is the concatenation
            uv = res["uv"].numpy()
            for mode in MODES:
                single = []
                for i, tm in enumerate(tmaps):
                    r1 = call(map_attr=tm if i else tm[None], render_uv=True, render_map_attr=True, grid_interpolate_mode=mode)      # [1,Ht,Wt,C] and [Ht,Wt,C]
                    assert r1["map_attr"].shape == (N_VIEWS, H, W, tm.shape[-1]) and torch.equal(r1["uv"], res["uv"])
                    single.append(r1["map_attr"])
                    fix["map_%d_%s_%s" % (i, mode, tag)] = r1["map_attr"].numpy()
                    outside, half = conditions(uv, cov, tm.shape[0], tm.shape[1])
                    assert outside[mode].any(), "no covered pixel of %s has a tap outside map %d in mode %s" % (tag, i, mode)
                    assert half.any(), "no covered pixel of %s lies on an exact half of map %d that rounds down to even" % (tag, i)
                both = call(map_attr=tuple(tmaps), render_uv=True, render_map_attr=True, grid_interpolate_mode=mode)["map_attr"]
                assert torch.equal(both, torch.cat(single, -1)), mode
                if mode == "bilinear":
                    assert torch.equal(both, res["map_attr"])
            # ---- the background forms: a float, a [C] tensor, a dense [B,H,W,C] tensor (None is above)
            r = call(v_attr=torch.from_numpy(v_attr7[:, :1].copy()), render_v_attr=True)
            fix["v_attr1_" + tag] = r["v_attr"].numpy()
            r = call(v_attr=torch.from_numpy(v_attr7[:, :4].copy()), render_v_attr=True, background=BG_FLOAT)
            fix["v_attr4_float_" + tag] = r["v_attr"].numpy()
            r = call(v_attr=torch.from_numpy(v_attr7), render_v_attr=True, background=bg_vec[7])
            fix["v_attr7_vec_" + tag] = r["v_attr"].numpy()
            r = call(v_attr=torch.from_numpy(v_attr7[:, :4].copy()), render_v_attr=True, background=bg_dense[4])
            fix["v_attr4_dense_" + tag] = r["v_attr"].numpy()
            for mode in MODES:
                r = call(map_attr=tuple(tmaps), render_uv=True, render_map_attr=True, grid_interpolate_mode=mode, background=BG_FLOAT)
                assert torch.equal(r["map_attr"][res["mask"][..., 0]], torch.from_numpy(np.concatenate(
                    [fix["map_%d_%s_%s" % (i, mode, tag)] for i in range(2)], -1))[res["mask"][..., 0]])
                assert (r["map_attr"][~res["mask"][..., 0]] == BG_FLOAT).all()
            r = call(map_attr=tmaps[0], render_uv=True, render_map_attr=True, background=bg_vec[3])
            fix["map_0_bilinear_vec_" + tag] = r["map_attr"].numpy()
            r = call(map_attr=tmaps[1], render_uv=True, render_map_attr=True, grid_interpolate_mode="nearest", background=bg_dense[5])
            fix["map_1_nearest_dense_" + tag] = r["map_attr"].numpy()
        # ---- the flags that stay unbuilt: what the reference does when they are set
        vox = torch.zeros(4, 4, 4, 3)
        for name, kw in (("voxel_attr", dict(render_world_position=True, render_voxel_attr=True)),
                         ("all_point_cloud", dict(render_all_point_cloud=True)), ("visible_point_cloud", dict(render_visible_point_cloud=True))):
            try:
                renderer.simple_rendering(mesh, None, None, vox, c2ws, intr, SCREEN, enable_antialis=False, **kw)
                fix["refusal_" + name] = np.array("")
            except Exception as e:      # noqa: BLE001 -- the type is the recorded result
                fix["refusal_" + name] = np.array(type(e).__name__)
            print("refusal", name, repr(str(fix["refusal_" + name])))
        # ---- atlas v_attr (simple_inverse_rendering :491-502) on the 48 x 40 atlas of G17, background 0.5
        log["rast"], log["attr"] = [], []
        res = renderer.simple_inverse_rendering(mesh, torch.from_numpy(v_attr7[:, :4].copy()), None, None, None, None, ATLAS, render_v_attr=True,
                                                background=0.5)
        assert sorted(res) == ["alpha", "mask", "v_attr"] and res["v_attr"].shape == (1,) + ATLAS + (4,)
        fix["atlas_rast"], fix["atlas_v_attr4_half"] = log["rast"][0][0], res["v_attr"].numpy()
        assert (res["v_attr"][~res["mask"][..., 0]] == 0.5).all() and res["mask"].any() and not res["mask"].all()
    finally:
        dr.rasterize, dr.interpolate = rast_fn, interp_fn
    assert all(v.dtype in (np.float32, np.int32) or v.dtype.kind == "U" for v in fix.values()), [k for k, v in fix.items() if v.dtype not in (np.float32, np.int32)]
    assert all(np.isfinite(v).all() for v in fix.values() if v.dtype == np.float32)
    path = os.path.join(out, "g18_simple_rendering.npz")
    np.savez_compressed(path, **fix)
    print("G18: %d arrays, %d bytes" % (len(fix), os.path.getsize(path)))
    assert os.path.getsize(path) < 1024 * 1024


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g18_simple_rendering(out)
    print("wrote g18_simple_rendering")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
