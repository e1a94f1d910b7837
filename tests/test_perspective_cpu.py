"""Perspective cameras in back-projection and the condition render, CPU side: the reference's perspective ray model restated in numpy float32
in the HIP kernels' operation order (utx_backproject_persp, utx_view_visibility_persp), the rest through the existing oracle (rasteriser,
interpolation, LBVH trace, visibility dilation), against the reference's own outputs (fixtures G67p / G11p / G9p,
tests/golden/make_golden_perspective.py).

Reference (TextureTools/texturetools/render/nvdiffrast/renderer_inverse.py): with perspective=True every ray of a view starts at the camera
centre c2w[:3, 3] and points at the surface point, rays_d = normalize(pos - rays_o) = x / max(|x|, 1e-12) (:187-190 view pixels, :279-285 texels);
a texel is seen when the closest hit is its own face and cosine_similarity(rays_d, face normal) < cos(threshold)."""
import math
import os

import numpy as np

from oracle import geom_ref as G

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


def load(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def unpack(a, shape):
    return np.unpackbits(a)[:int(np.prod(shape))].reshape(shape).astype(bool)


def persp_dirs(pos, eye):
    """pos [..., 3], eye [3] -> (pos - eye) / max(sqrt((x*x + y*y) + z*z), 1e-12), float32, the kernels' order"""
    pos, eye = np.asarray(pos, F32), np.asarray(eye, F32)
    x, y, z = pos[..., 0] - eye[0], pos[..., 1] - eye[1], pos[..., 2] - eye[2]
    n = np.maximum(np.sqrt((x * x + y * y) + z * z), F32(1e-12))
    return np.stack([x / n, y / n, z / n], -1).astype(F32)


def facing(d, fn, angle_deg):
    """cosine_similarity(d, fn) < cos(angle) with eps 1e-8 on both norms: the shared cosine expression of the kernels"""
    d, fn = np.asarray(d, F32), np.asarray(fn, F32)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    ld = np.maximum(np.sqrt(dot(d, d)), F32(1e-8))
    ln = np.maximum(np.sqrt(dot(fn, fn)), F32(1e-8))
    return (dot(d, fn) / (ld * ln)) < F32(math.cos(math.radians(angle_deg)))


def texel_rayvis(rast2d, verts, faces, fn, eyes, bvh, angle_deg):
    """uv_to_pcd's per-texel ray test with perspective rays -> rayvis [n, Th, Tw] u8 (before the hole filling)"""
    cov = rast2d[..., 3] > 0
    tid = rast2d[..., 3].astype(np.int64)[cov] - 1
    pos = G.interpolate(verts, rast2d, faces)[cov]
    out = np.zeros((len(eyes),) + cov.shape, np.uint8)
    for v, eye in enumerate(np.asarray(eyes, F32)):
        d = persp_dirs(pos, eye)
        hit = bvh.trace(np.broadcast_to(eye, d.shape), d)
        out[v][cov] = ((hit == tid) & (hit != -1) & facing(d, fn[tid], angle_deg)).astype(np.uint8)
    return out


def view_visibility_persp(attr6, rast, fn, eyes, grad_thr=0.20, angle_deg=115.0):
    """mv_to_pcd(filt_gradient_points=True) with perspective rays: coverage AND the eroded gradient test (the oracle's view_visibility, its
    facing term switched off by zero face normals -- cosine 0 -- and an 80 degree threshold) AND the perspective facing test"""
    smooth_cov = G.view_visibility(attr6, rast, np.zeros_like(fn), np.ones((len(eyes), 3), F32), grad_thr=grad_thr, angle_deg=80.0)
    tid = np.maximum(rast[..., 3].astype(np.int64) - 1, 0)
    face = np.stack([facing(persp_dirs(attr6[v, ..., :3], e), fn[tid[v]], angle_deg) for v, e in enumerate(np.asarray(eyes, F32))])
    return smooth_cov & face


def scene(f):
    verts, faces, uvs, c2ws, intr = f["verts"], f["faces"], f["uvs"], f["c2ws"], f["intr"]
    clip = G.transform_points(verts, G.mvp_matrices(c2ws, intr, perspective=True))
    uvclip = np.concatenate([uvs * 2 - 1, np.zeros((len(uvs), 1), F32), np.ones((len(uvs), 1), F32)], -1)
    return dict(verts=verts, faces=faces, clip=clip, vndc=(clip[..., :2] / clip[..., 3:4]).astype(F32), uvclip=uvclip,
                fn=G.face_normals(verts, faces), eyes=np.ascontiguousarray(c2ws[:, :3, 3], F32), dirs=(-c2ws[:, :3, 2]).astype(F32))


def atlas_visibility(s, T, images4, angle_deg):
    """(rast2d, rayvis, alphaok, colour, dilated visibility) of uv_to_pcd with perspective rays; colour and alpha do not depend on the rays and
    come from the oracle's gather"""
    rast2d = G.rasterize(s["uvclip"], s["faces"], T, T)
    bvh = G.BVH(s["verts"], s["faces"])
    col, _, ao = G.backproject(rast2d, s["verts"], s["faces"], s["fn"], s["vndc"], s["dirs"], images4, bvh, angle_deg=angle_deg)
    rv = texel_rayvis(rast2d, s["verts"], s["faces"], s["fn"], s["eyes"], bvh, angle_deg)
    return rast2d, rv, ao, col, G.dilate_visibility(rv, rast2d[..., 3] > 0, ao)


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
