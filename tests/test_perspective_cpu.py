"""Perspective cameras in back-projection and the condition render, CPU side: the reference's perspective ray model restated in numpy float32
in the HIP kernels' operation order (oracle/reproject_ref.py: utx_backproject_persp, utx_view_visibility_persp), the rest through the existing
oracle (rasteriser, interpolation, LBVH trace, visibility dilation), against the reference's own outputs (fixtures G67p / G11p / G9p,
tests/golden/make_golden_perspective.py)."""
import numpy as np

from oracle import geom_ref as G
from oracle.reproject_ref import F32, atlas_visibility, load, scene, unpack, view_visibility_persp


def test_g67p_perspective_texel_visibility_matches_reference():
    f = load("g67p_backprojection_perspective.npz")
    s = scene(f)
    imgs = f["images"].astype(F32)
    n, HW = imgs.shape[:2]
    T = 96
    mv_alpha = np.stack([G.rasterize(s["clip"][v], s["faces"], HW, HW)[..., 3] > 0 for v in range(n)])
    assert np.array_equal(mv_alpha, unpack(f["mv_alpha"], (n, HW, HW, 1))[..., 0]), "perspective view coverage"
    alpha = unpack(f["alpha"], (n, HW, HW, 1)).astype(F32)
    rast2d, rv, ao, col, vis = atlas_visibility(s, T, np.concatenate([imgs, alpha], -1), 100.0)
    assert np.array_equal(rast2d[..., 3] > 0, unpack(f["mask_2d"], (1, T, T, 1))[0, ..., 0])
    ref = unpack(f["mask_2d_visiable"], (n, T, T, 1))[..., 0]
    mism = int((vis != ref).sum())
    print("G67p texel visibility: %d of %d differ; visible per view %s" % (mism, ref.size, ref.sum((1, 2)).tolist()))
    assert mism <= 4
    assert ref.sum() > 5000 and (ref.sum((1, 2)) > 1000).all()
    # the rays matter: the orthographic model on the same cameras sees another set of texels
    _, rv_ortho, _ = G.backproject(rast2d, s["verts"], s["faces"], s["fn"], s["vndc"], s["dirs"], np.concatenate([imgs, alpha], -1),
                                   G.BVH(s["verts"], s["faces"]), angle_deg=100.0)
    assert int((G.dilate_visibility(rv_ortho, rast2d[..., 3] > 0, ao) != ref).sum()) > 20 * max(mism, 1)
    both = vis & ref
    ref_cols = np.zeros((n, T, T, 3), F32)
    ref_cols[ref] = f["vis_colors"]
    assert np.abs(ref_cols[both] - col[both]).max() < 2e-6, "gathered colours at the perspective NDC"


def test_g11p_perspective_gradient_filter_matches_reference():
    f = load("g11p_filter_and_kdtree_perspective.npz")
    s = scene(f)
    imgs = f["images"].astype(F32)
    n, HW = imgs.shape[:2]
    T = 96
    va = np.concatenate([s["verts"], G.vertex_normals_area(s["verts"], s["faces"])], -1).astype(F32)
    rast = np.stack([G.rasterize(s["clip"][v], s["faces"], HW, HW) for v in range(n)])
    assert np.array_equal(rast[..., 3] > 0, unpack(f["mask"], (n, HW, HW, 1))[..., 0])
    attr = np.stack([G.interpolate(va, rast[v], s["faces"]) for v in range(n)])
    vis = view_visibility_persp(attr, rast, s["fn"], s["eyes"])
    ref = unpack(f["mask_visiable"], (n, HW, HW, 1))[..., 0]
    mism = int((vis != ref).sum())
    print("G11p filtered view masks: %d of %d differ; %d visible" % (mism, ref.size, int(ref.sum())))
    assert mism <= 8
    assert 1000 < ref.sum() < 0.5 * rast[..., 3].astype(bool).sum()
    # texels, with the reference's view masks as the alpha
    _, _, _, _, v2d = atlas_visibility(s, T, np.concatenate([imgs, ref[..., None].astype(F32)], -1), 115.0)
    ref2d = unpack(f["mask_2d_visiable"], (n, T, T, 1))[..., 0]
    assert int((v2d != ref2d).sum()) <= 4 and ref2d.sum() > 500


def test_g9p_condition_cameras_match_reference():
    from unitex_amd.texturetools.video import condition_cameras
    f = load("g9p_export_condition_perspective.npz")
    c2ws, intr = condition_cameras(4, 2, 2, scale=1.0, fov_deg=49.1, perspective=True, orbit=True)
    assert np.array_equal(c2ws.numpy(), f["c2ws"]) and np.array_equal(intr.numpy(), f["intrinsics"])
    # orbit=False keeps the box views (fixture G9), any n_views = n_rows * n_cols on the ring
    g9 = load("g9_export_condition.npz")
    c2ws, intr = condition_cameras(6, 2, 3, scale=1.0, perspective=False, orbit=False)
    assert np.array_equal(c2ws.numpy(), g9["c2ws"]) and np.array_equal(intr.numpy(), g9["intrinsics"])
    c2ws, _ = condition_cameras(9, 3, 3, orbit=True)
    assert c2ws.shape == (9, 4, 4) and np.allclose(np.linalg.norm(c2ws[:, :3, 3].numpy(), axis=-1), 2.8, atol=1e-5)
