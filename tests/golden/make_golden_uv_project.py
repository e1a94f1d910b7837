#!/usr/bin/env python
"""Generate the atlas-space view-projection fixture under tests/golden/ from the REFERENCE's own Python, through the same seams as make_golden.py
(imported from there, unchanged):

    python tests/golden/make_golden_uv_project.py            # writes tests/golden/g19_uv_project.npz

  G19   NVDiffRendererBase.simple_inverse_rendering(render_uv=True, render_map_attr=True, enable_antialis=False)
        (render/nvdiffrast/renderer_base.py:504-559), Mesh.get_visible_faces / get_visible_vertices (mesh/structure.py:801-857),
        NVDiffRendererBase.get_visible_faces / get_visible_vertices (renderer_base.py:65-99) and erode_face (topology.py:12-25): all the reference's own.
Seams: dr.rasterize / dr.interpolate -> the build's CPU rasteriser (oracle/geom_ref.c); dr.antialias is STUBBED to return its first argument;
dr.texture -> the restatement of nvdiffrast's linear lookup with the wrap boundary that G67n uses; F.grid_sample is torch's own.  The `open3d` stub
gains a RaycastingScene whose cast_rays is NOT Embree but a SEAM written here: a brute force in float64 (tests/uv_project_ref.closest_hit: every ray
against every triangle, Moeller-Trumbore on both sides, the smallest t >= 0, ties to the lowest id).  The scene is chosen so that this cannot matter:
for every ray the winner leads the next hit by more than 1e-4 in t and no candidate hit lies within 1e-4 of a triangle's edge (asserted below), which
is about a hundred times the rounding of a float32 intersector.
Scene: the two-chart cylinder of G17 (its v range moved up to make room) plus a detached plate of two triangles with a UV chart of its own, standing
inside the open shell, between camera 0 and the far chart, where every view of both sets sees it through a gap; atlas 48 x 40; both camera sets of G17 (B = 3); maps 16 x 24 x 3 and 8 x 8 x 5, each shared ([1,...]) and
one per view ([B,...]); the three filters; the background forms None, a float, a [C] vector and a dense [B,H,W,C] image.
Asserted per camera set and view: some faces are hidden by the cylinder itself, some ray marks a face other than the one it was aimed at, some faces are hidden by the plate; per
camera set: some texels have vis true but cov < 1 (the views rasterised at 8 x 8 lose thin coverage).  The outside-tap condition of G18
(visible texels with a tap outside the map, per filter and map) is asserted too: the cameras keep G17's c2ws but frame the mesh more tightly
(INTRINSICS below), so uv reaches past the maps' borders.  G18's exact-half condition is NOT met and not asserted: uv is the interpolated NDC of a real
projection, and no visible texel of this scene lands on an exact half of a 8-, 16- or 24-texel axis (the maker prints the count: 0);
tests/test_uv_project_gpu.py reaches exact halves with a v_ndc of its own, against this build's screen-kernel lookup only.
The combination render_uv + a camera-dependent geometry flag is MADE and what the reference does is stored (refusal_uv_with_camera_flags).
Stored: mesh, cameras, the atlas raster, the views' rasters at both map sizes, v_ndc, face and vertex masks of both methods with erode_neighbor 0 and
1, every output.  float32 / int32 / uint8 / text, exact; data only."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ROOT, _make_inverse_renderer, install_stubs  # noqa: E402
from make_golden_reproject_variants import nvdiffrast_texture_linear_wrap  # noqa: E402
from make_golden_simple_rendering import _cameras, _renderer, conditions  # noqa: E402
from make_golden_uv_maps import ATLAS, N_VIEWS, SETS, _two_charts  # noqa: E402

sys.path.insert(0, ROOT)
from oracle import uv_project_ref as REFN  # noqa: E402

MODES = ("bilinear", "nearest", "nvdiffrast")
MAP_SHAPES = ((16, 24, 3), (8, 8, 5))
RASTER_SIZE = (40, 56)                                  # the raster method's render_size
BG_FLOAT = 0.25
# G17's rings (c2ws) with a narrower frame than G17's intrinsics (fov 49.1 deg, scale 0.85), so that the mesh reaches the border of the view and uv the
# border of the maps: (fov in degrees, perspective) and (scale, orthographic).  The rays do not read the intrinsics.
INTRINSICS = {"p": (28.0, 28.0, True), "o": (1.4, 1.4, False)}
# the plate: a quad of two triangles, corners in order; found by a search over placements for the margin and the conditions asserted below
PLATE = np.array([[-0.131, -0.734, 0.008], [0.584, -0.523, 0.019], [0.710, 0.146, -0.088], [-0.034, -0.022, -0.107]], np.float32)
PLATE_UV = np.array([[0.15, 0.03], [0.60, 0.03], [0.60, 0.15], [0.15, 0.15]], np.float32)


def scene():
    verts, faces, uvs, nrm = _two_charts()
    uvs = uvs.copy()
    uvs[:, 1] = (0.2 + (uvs[:, 1].astype(np.float64) - 0.08) * (0.74 / 0.86)).astype(np.float32)
    n = verts.shape[0]
    pn = np.cross(PLATE[1] - PLATE[0], PLATE[3] - PLATE[0])
    verts = np.concatenate([verts, PLATE])
    faces = np.concatenate([faces, np.array([[n, n + 1, n + 2], [n, n + 2, n + 3]], np.int32)])
    uvs = np.concatenate([uvs, PLATE_UV])
    nrm = np.concatenate([nrm, np.tile((pn / np.linalg.norm(pn)).astype(np.float32), (4, 1))])
    return verts.astype(np.float32), faces.astype(np.int32), uvs.astype(np.float32), nrm.astype(np.float32)


class _Ids:
    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a


class RaycastingScene:
    """SEAM, not Embree: float64 brute-force closest hit (module docstring).  `margins` collects, per cast, the rays that pass the margin."""
    INVALID_ID = 4294967295
    margins = []

    def add_triangles(self, mesh):
        self.verts, self.faces = mesh

    def cast_rays(self, rays):
        rays = np.asarray(rays)
        hit, ok = REFN.closest_hit(self.verts, self.faces, rays[:, :3], rays[:, 3:])
        RaycastingScene.margins.append(ok)
        return {"primitive_ids": _Ids(np.where(hit < 0, self.INVALID_ID, hit).astype(np.uint32))}


def install_open3d_seam():
    o3d = importlib.import_module("open3d")
    o3d.t = types.SimpleNamespace(geometry=types.SimpleNamespace(RaycastingScene=RaycastingScene,
                                                                 TriangleMesh=types.SimpleNamespace(from_legacy=lambda m, **k: m)))
    o3d.core = types.SimpleNamespace(Tensor=lambda a, dtype=None, device=None: a, float32="float32", int64="int64", Device=lambda s: s)


def g19_uv_project(out):
    _make_inverse_renderer()           # installs the dr stubs (rasterize / interpolate -> oracle)
    dr = importlib.import_module("nvdiffrast.torch")
    S = importlib.import_module("TextureTools.texturetools.mesh.structure")
    T = importlib.import_module("TextureTools.texturetools.geometry.triangle_topology.topology")
    install_open3d_seam()
    gen = importlib.import_module("TextureTools.texturetools.camera.generator")
    RB = importlib.import_module("TextureTools.texturetools.render.nvdiffrast.renderer_base")
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

    verts, faces, uvs, nrm = scene()
    F, V = faces.shape[0], verts.shape[0]
    H, W = ATLAS
    mesh = types.SimpleNamespace(v_pos=torch.from_numpy(verts), v_nrm=torch.from_numpy(nrm), t_pos_idx=torch.from_numpy(faces).long(),
                                 v_tex=torch.from_numpy(uvs), t_tex_idx=torch.from_numpy(faces).long(), device=torch.device("cpu"),
                                 to_open3d=lambda: (verts, faces))
    mesh.get_visible_faces = lambda c2ws, perspective=True: S.Mesh.get_visible_faces(mesh, c2ws, perspective=perspective)
    fix = dict(verts=verts, faces=faces, uvs=uvs, v_nrm=nrm)
    rng = np.random.default_rng(19)
    maps = [rng.uniform(0.0, 1.0, (N_VIEWS,) + s).astype(np.float16).astype(np.float32) for s in MAP_SHAPES]      # [B,...]; the shared map is [0:1]
    fix.update(map_0=maps[0], map_1=maps[1], bg_float=np.float32(BG_FLOAT))
    bg_vec = {c: rng.uniform(0.0, 1.0, c).astype(np.float32) for c in (3, 5)}
    bb, yy, xx, cc = np.meshgrid(np.arange(N_VIEWS), np.arange(H), np.arange(W), np.arange(5), indexing="ij")
    dense = (((5 * bb + 3 * yy + xx + 7 * cc) % 16) / 16.0).astype(np.float32)
    fix.update(bg_vec_3=bg_vec[3], bg_vec_5=bg_vec[5], bg_dense_5=dense, bg_dense_3=dense[..., :3].copy())
    is_plate = np.arange(F) >= F - 2
    try:
        for tag, perspective, height, theta_0 in SETS:
            renderer = _renderer(RB, perspective)
            c2ws, _ = _cameras(gen, perspective, height, theta_0)
            intr = gen.generate_intrinsics(*INTRINSICS[tag][:2], fov=INTRINSICS[tag][2], degree=INTRINSICS[tag][2])
            fix["c2ws_" + tag], fix["intr_" + tag] = c2ws.numpy().astype(np.float32), intr.numpy().astype(np.float32)
            # ---- visibility: rays (Mesh.get_visible_faces), raster (NVDiffRendererBase.get_visible_faces), erode 0 / 1, vertices
            RaycastingScene.margins = []
            m_rays = S.Mesh.get_visible_faces(mesh, c2ws, perspective=perspective)
            ok = RaycastingScene.margins[0]
            assert ok.all(), "%s: %d rays fail the margin: move the plate" % (tag, int((~ok).sum()))
            mask_np, hit, _ = REFN.visible_faces_rays(verts, faces, fix["c2ws_" + tag], perspective)
            assert np.array_equal(mask_np, m_rays.numpy())
            aimed = np.arange(F)[None]
            for b in range(N_VIEWS):
                other = (hit[b] != aimed[0]) & (hit[b] >= 0)
                assert other.any(), "%s view %d: every ray marks the face it was aimed at" % (tag, b)
                assert (other & ~is_plate[np.clip(hit[b], 0, None)] & ~is_plate).any(), "%s view %d: no face hidden by the cylinder itself" % (tag, b)
            by_plate = (hit >= 0) & is_plate[np.clip(hit, 0, None)] & ~is_plate[None]
            assert by_plate.any(1).all(), "%s: a view without a face hidden by the plate: %s" % (tag, by_plate.sum(1))
            print("G19 %s: faces hidden by the plate per view %s, rays marking another face %s, visible faces %s" %
                  (tag, by_plate.sum(1).tolist(), ((hit != aimed) & (hit >= 0)).sum(1).tolist(), mask_np.sum(1).tolist()))
            fix["faces_rays_e0_" + tag] = m_rays.numpy().astype(np.uint8)
            m_rays1 = torch.stack([T.erode_face(mesh.t_pos_idx, m_rays[b], V, 1) for b in range(N_VIEWS)])
            fix["faces_rays_e1_" + tag] = m_rays1.numpy().astype(np.uint8)
            fix["verts_rays_e0_" + tag] = S.Mesh.get_visible_vertices(mesh, c2ws, perspective=perspective).numpy().astype(np.uint8)
            for e in (0, 1):
                renderer.erode_neighbor = e
                log["rast"] = []
                fix["faces_raster_e%d_%s" % (e, tag)] = renderer.get_visible_faces(mesh, c2ws, intr, RASTER_SIZE).numpy().astype(np.uint8)
                fix["verts_raster_e%d_%s" % (e, tag)] = renderer.get_visible_vertices(mesh, c2ws, intr, RASTER_SIZE).numpy().astype(np.uint8)
                fix["rast_view_" + tag] = log["rast"][0]
            renderer.erode_neighbor = 0
            assert fix["faces_rays_e1_" + tag].sum() < fix["faces_rays_e0_" + tag].sum() and fix["faces_rays_e1_" + tag].any()
            assert fix["faces_raster_e1_" + tag].sum() < fix["faces_raster_e0_" + tag].sum() and fix["faces_raster_e1_" + tag].any()
            # ---- the projection
            call = lambda m, **kw: renderer.simple_inverse_rendering(mesh, None, m, None, c2ws, intr, ATLAS, render_uv=True, enable_antialis=False, **kw)
            log["rast"], log["attr"] = [], []
            res = call(None)
            assert sorted(res) == ["alpha", "mask", "uv", "uv_alpha"] and len(log["rast"]) == 1 and len(log["attr"]) == 1
            fix["rast2d"], fix["v_ndc_" + tag] = log["rast"][0][0], log["attr"][0]
            assert fix["v_ndc_" + tag].shape == (N_VIEWS, V, 2) and res["uv"].shape == (N_VIEWS, H, W, 2) and res["uv_alpha"].shape == (N_VIEWS, H, W, 1)
            fix["uv_" + tag], fix["uv_alpha_" + tag] = res["uv"].numpy(), res["uv_alpha"].numpy()
            vis = res["uv_alpha"].numpy()[..., 0] > 0
            assert vis.reshape(N_VIEWS, -1).any(1).all()
            for shape in MAP_SHAPES:      # the outside-tap condition of G18, per filter and map, on the texels the views see
                outside, half = conditions(res["uv"].numpy(), vis, shape[0], shape[1])
                for mode in MODES:
                    assert outside[mode].any(), "no visible texel of %s has a tap outside the %d x %d map in mode %s" % (tag, shape[0], shape[1], mode)
                print("G19 %s, map %d x %d: visible texels with a tap outside %s, on an exact half %d; max |uv| %s" % (
                    tag, shape[0], shape[1], {k: int(v.sum()) for k, v in outside.items()}, int(half.sum()), np.abs(res["uv"].numpy()[vis]).max(0)))
            lost = 0
            for i, shape in enumerate(MAP_SHAPES):
                for per_view in (False, True):
                    tm = torch.from_numpy(maps[i] if per_view else maps[i][:1])
                    for mode in MODES:
                        log["rast"] = []
                        r = call(tm, render_map_attr=True, grid_interpolate_mode=mode)
                        key = "map_%d_%s_%s_%s" % (i, "b" if per_view else "1", mode, tag)
                        assert r["map_attr"].shape == (N_VIEWS, H, W, shape[2]) and torch.equal(r["uv"], res["uv"])
                        fix[key], fix["uv_alpha_map_%d_%s" % (i, tag)] = r["map_attr"].numpy(), r["uv_alpha"].numpy()
                        fix["rast_map_%d_%s" % (i, tag)] = log["rast"][1]
                        assert log["rast"][1].shape == (N_VIEWS,) + shape[:2] + (4,)
                    lost += int((vis & (fix["uv_alpha_map_%d_%s" % (i, tag)][..., 0] < 1)).sum())
            assert lost > 0, "%s: no texel with vis true but cov < 1" % tag
            # ---- the background forms: a float, a [C] vector, a dense [B,H,W,C] image (None is above)
            c0, c1 = MAP_SHAPES[0][2], MAP_SHAPES[1][2]
            fix["map_0_1_bilinear_float_" + tag] = call(torch.from_numpy(maps[0][:1]), render_map_attr=True, background=BG_FLOAT)["map_attr"].numpy()
            fix["map_1_b_nearest_vec_" + tag] = call(torch.from_numpy(maps[1]), render_map_attr=True, grid_interpolate_mode="nearest",
                                                     background=torch.from_numpy(bg_vec[c1]))["map_attr"].numpy()
            fix["map_0_b_nvdiffrast_dense_" + tag] = call(torch.from_numpy(maps[0]), render_map_attr=True, grid_interpolate_mode="nvdiffrast",
                                                          background=torch.from_numpy(dense[..., :c0].copy()))["map_attr"].numpy()
            fix["map_1_1_bilinear_vec_" + tag] = call(torch.from_numpy(maps[1][:1]), render_map_attr=True,
                                                      background=torch.from_numpy(bg_vec[c1]))["map_attr"].numpy()
        # ---- what the reference does with render_uv + a camera-dependent geometry flag (:446 rebinds batch_size), and without cameras
        for name, args, kw in (("uv_with_camera_flags", (c2ws, intr), dict(render_uv=True, render_camera_position=True)),
                               ("uv_without_cameras", (None, None), dict(render_uv=True)),
                               ("map_attr_without_uv", (c2ws, intr), dict(render_map_attr=True))):
            try:
                r = renderer.simple_inverse_rendering(mesh, None, torch.from_numpy(maps[0][:1]), None, args[0], args[1], ATLAS, enable_antialis=False, **kw)
                fix["refusal_" + name] = np.array("" if name != "map_attr_without_uv" else ",".join(sorted(r)))
            except Exception as e:      # noqa: BLE001 -- the type is the recorded result
                fix["refusal_" + name] = np.array(type(e).__name__)
            print("refusal", name, repr(str(fix["refusal_" + name])))
    finally:
        dr.rasterize, dr.interpolate = rast_fn, interp_fn
    assert all(v.dtype in (np.float32, np.int32, np.uint8) or v.dtype.kind == "U" for v in fix.values()), [k for k, v in fix.items() if v.dtype.kind not in "fiuU"]
    assert all(np.isfinite(v).all() for v in fix.values() if v.dtype == np.float32)
    path = os.path.join(out, "g19_uv_project.npz")
    np.savez_compressed(path, **fix)
    print("G19: %d arrays, %d bytes" % (len(fix), os.path.getsize(path)))
    assert os.path.getsize(path) < 1024 * 1024


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g19_uv_project(out)
    print("wrote g19_uv_project")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
