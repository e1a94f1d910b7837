#!/usr/bin/env python
"""Generate the perspective-camera fixtures under tests/golden/ from the REFERENCE's own Python, through the same seams as
make_golden.py (imported from there, unchanged):

    python tests/golden/make_golden_perspective.py            # writes tests/golden/g67p_*.npz, g11p_*.npz, g9p_*.npz

  G67p  mv_to_pcd + uv_to_pcd + bake_mv_to_uv_reproject_blur with perspective=True (renderer_inverse.py:159-343, 574-633): fov 49.1 deg,
        the box cameras at radius 2.8, 48^2 views, a 96^2 atlas, the view alpha holed as in G6/G7.
  G11p  mv_to_pcd(filt_gradient_points=True) + bake_mv_to_uv_kdtree('order_mean') with perspective=True at 96^2 views (at 48^2 the filter
        leaves no view pixel and the reference's bake raises IndexError).
  G9p   VideoExporter.export_condition(orbit=True, perspective=True, n_views=4, 2 x 2) at 64^2 (export_nvdiffrast_video.py:900-999).
Masks are stored with np.packbits, images as float16 (the inputs are rounded to half first, so they are exact)."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _make_inverse_renderer, _sphere, install_stubs  # noqa: E402

FOV = 49.1


def _views(HW, seed, fx, fy):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, HW), np.linspace(0, 1, HW), indexing="ij")
    imgs = np.zeros((6, HW, HW, 3), np.float32)
    for v in range(6):
        ph = rng.uniform(0, 6.28, 6)
        for c in range(3):
            imgs[v, ..., c] = 0.5 + 0.5 * np.sin(fx * xx + ph[c]) * np.cos(fy * yy + ph[c + 3])
    return imgs.astype(np.float16).astype(np.float32), xx, yy


def _cameras():
    gen = importlib.import_module("TextureTools.texturetools.camera.generator")
    c2ws = gen.generate_box_views_c2ws(2.8)[[0, 1, 4, 2, 3, 5]]
    intr = gen.generate_intrinsics(FOV, FOV, fov=True, degree=True)
    return c2ws, intr


def g67p_backprojection(out):
    inv, R, (verts, faces, uvs) = _make_inverse_renderer()
    c2ws, intr = _cameras()
    HW, T = 48, 96
    imgs, xx, yy = _views(HW, 31, 7, 5)
    image_attrs = torch.from_numpy(imgs)
    with torch.no_grad():
        mv = inv.mv_to_pcd(c2ws, intr, (HW, HW), image_attrs=image_attrs, perspective=True, filt_gradient_points=False)
        hole = torch.from_numpy((((xx - 0.5) ** 2 + (yy - 0.5) ** 2) > 0.16 ** 2) | (xx < 0.3)).float()[None, :, :, None]
        alpha = mv["alpha_visiable"].clone() * hole
        uv = inv.uv_to_pcd(c2ws, intr, (T, T), image_attrs=image_attrs, alpha_attrs=alpha, perspective=True, ray_normal_angle_threhold=100)
        bake = inv.bake_mv_to_uv_reproject_blur(uv["point_cloud_2d_visiable"], uv["point_cloud_2d"], uv["mask_2d_visiable"],
                                                uv["mask_2d"], method="lens")
    print("G67p: covered %d, visible per view %s" % (int(uv["mask_2d"].sum()), uv["mask_2d_visiable"].sum((1, 2, 3)).tolist()))
    np.savez_compressed(os.path.join(out, "g67p_backprojection_perspective.npz"), verts=verts, faces=faces, uvs=uvs, c2ws=c2ws.numpy(),
                        intr=intr.numpy(), images=imgs.astype(np.float16), alpha=np.packbits(alpha.numpy() > 0),
                        mv_alpha=np.packbits(mv["alpha"].numpy() > 0), mask_2d=np.packbits(uv["mask_2d"].numpy()),
                        mask_2d_visiable=np.packbits(uv["mask_2d_visiable"].numpy()),
                        vis_colors=uv["point_cloud_2d_visiable"].colors.numpy(), color_2d=bake["color_2d"].numpy())


def g11p_filter_and_kdtree(out):
    inv, R, (verts, faces, uvs) = _make_inverse_renderer()

    def knn_sq(src, dst, k=1, **kw):      # squared distances, as torch_kdtree (make_golden.g11_kdtree_and_filter)
        from scipy.spatial import cKDTree
        d, i = cKDTree(src.numpy().astype(np.float64)).query(dst.numpy().astype(np.float64), k=k)
        i = torch.from_numpy(np.asarray(i).reshape(dst.shape[0], k)).long()
        return torch.from_numpy(np.asarray(d).reshape(dst.shape[0], k) ** 2).float(), i
    R.knn = knn_sq
    c2ws, intr = _cameras()
    HW, T = 96, 96
    imgs, _, _ = _views(HW, 33, 6, 4)
    image_attrs = torch.from_numpy(imgs)
    fix = dict(verts=verts, faces=faces, uvs=uvs, c2ws=c2ws.numpy(), intr=intr.numpy(), images=imgs.astype(np.float16))
    with torch.no_grad():
        mv = inv.mv_to_pcd(c2ws, intr, (HW, HW), image_attrs=image_attrs, perspective=True, grad_norm_threhold=0.20,
                           ray_normal_angle_threhold=115.0, filt_gradient_points=True)
        fix["mask"] = np.packbits(mv["mask"].numpy())
        fix["mask_visiable"] = np.packbits(mv["mask_visiable"].numpy())
        print("G11p view mask: covered %d, visible after filter %d" % (int(mv["mask"].sum()), int(mv["mask_visiable"].sum())))
        uv = inv.uv_to_pcd(c2ws, intr, (T, T), image_attrs=image_attrs, alpha_attrs=mv["alpha_visiable"], perspective=True,
                           ray_normal_angle_threhold=115.0)
        fix["mask_2d"] = np.packbits(uv["mask_2d"].numpy())
        fix["mask_2d_visiable"] = np.packbits(uv["mask_2d_visiable"].numpy())
        print("G11p atlas: covered %d, visible per view %s" % (int(uv["mask_2d"].sum()), uv["mask_2d_visiable"].sum((1, 2, 3)).tolist()))
        bake = inv.bake_mv_to_uv_kdtree(mv["point_cloud_visiable"], uv["point_cloud_2d"], uv["mask_2d"], mv["mask_visiable"],
                                        uv["mask_2d_visiable"], method="order_mean", n_neighbors_visiable=1, n_neighbors_invisiable=4)
        fix["color_2d_order_mean"] = bake["color_2d"].numpy().astype(np.float32)
    np.savez_compressed(os.path.join(out, "g11p_filter_and_kdtree_perspective.npz"), **fix)


def g9p_export_condition(out):
    _make_inverse_renderer()           # installs the dr stubs (rasterize / interpolate -> oracle)
    V = importlib.import_module("TextureTools.texturetools.video.export_nvdiffrast_video")
    S = importlib.import_module("TextureTools.texturetools.mesh.structure")
    RB = importlib.import_module("TextureTools.texturetools.render.nvdiffrast.renderer_base")
    verts, faces, _ = _sphere()
    verts = (verts * np.array([1.3, 0.8, 1.0], np.float32) + np.array([0.2, -0.1, 0.05], np.float32)).astype(np.float32)
    ref_mesh = S.Mesh(v_pos=torch.from_numpy(verts), t_pos_idx=torch.from_numpy(faces).long())
    V.load_whole_mesh = lambda p: "in-memory"
    V.Texture = types.SimpleNamespace(from_trimesh=lambda m: types.SimpleNamespace(mesh=ref_mesh))
    orig_to = torch.Tensor.to

    def to_cpu(self, *a, **k):         # the reference moves everything to 'cuda'
        is_cuda = lambda x: (isinstance(x, str) and x.startswith("cuda")) or (isinstance(x, torch.device) and x.type == "cuda")
        a = tuple("cpu" if is_cuda(x) else x for x in a)
        if is_cuda(k.get("device")):
            k["device"] = "cpu"
        return orig_to(self, *a, **k)
    torch.Tensor.to = to_cpu
    try:
        fake_self = types.SimpleNamespace(mesh_renderer=RB.NVDiffRendererBase(device="cpu"))
        res = V.VideoExporter.export_condition(fake_self, "mesh.obj", geometry_scale=0.95, n_views=4, n_rows=2, n_cols=2, H=64, W=64,
                                               fov_deg=FOV, scale=1.0, perspective=True, orbit=True, background="grey",
                                               return_image=True, return_camera=True)
    finally:
        torch.Tensor.to = orig_to
    np.savez_compressed(os.path.join(out, "g9p_export_condition_perspective.npz"), verts=verts, faces=faces,
                        alpha=np.asarray(res["alpha"]), ccm=np.asarray(res["ccm"]), normal=np.asarray(res["normal"]),
                        c2ws=res["c2ws"].numpy(), intrinsics=res["intrinsics"].numpy())


def main():
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    only = set(sys.argv[1:])
    for fn in (g67p_backprojection, g11p_filter_and_kdtree, g9p_export_condition):
        if only and fn.__name__ not in only:
            continue
        fn(HERE)
        print("wrote", fn.__name__)


if __name__ == "__main__":
    main()
