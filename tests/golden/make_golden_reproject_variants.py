#!/usr/bin/env python
"""Generate the back-projection variant fixtures under tests/golden/ from the REFERENCE's own Python (uv_to_pcd, bake_mv_to_uv_reproject_blur),
through the same seams as make_golden.py (imported from there, unchanged) plus two more:

    python tests/golden/make_golden_reproject_variants.py     # writes tests/golden/g67g_*.npz, g67n_*.npz

  G67g  bake_mv_to_uv_reproject_blur(method='gaussian') at the default sizes (3 / 3 / 5) and at kernel_size_boundary=5,
        kernel_size_boundary_blur=5, kernel_size_blur=7, with the lens run beside each; the G67p scene (perspective box cameras at 2.8,
        fov 49.1, 48^2 views, a 96^2 atlas, the view alpha holed as in G67p).
  G67n  uv_to_pcd(grid_interpolate_mode='nvdiff') + the lens bake, one orthographic and one perspective set, with the cameras close enough
        that the sphere crosses every view border (there nvdiffrast's wrap boundary and grid_sample's zero padding disagree).

Third-party code behind the two extra seams, restated below (neither package is installed here):
  * nvdiffrast dr.texture(tex, uv, filter_mode='linear') with its default boundary_mode='wrap' (indexTextureLinear + bilerp);
  * torchvision.transforms.functional.gaussian_blur(img, kernel_size, sigma=None) (_get_gaussian_kernel1d / 2d, reflect pad, depthwise conv2d).
Masks are stored with np.packbits, images as float16 (the inputs are rounded to half first, so they are exact)."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _make_inverse_renderer, install_stubs  # noqa: E402

FOV = 49.1


# ---------------------------------------------------------------------------------------------------
# restatements of third-party code (the seams)
# ---------------------------------------------------------------------------------------------------
def nvdiffrast_texture_linear_wrap(tex, uv, filter_mode="linear", boundary_mode="wrap", **kw):
    """restates nvdiffrast's dr.texture for a 2-D texture, filter_mode='linear', boundary_mode='wrap' (texture.cu: indexTextureLinear + bilerp):
    u -= floor(u); u = u * W - 0.5; i0 = floor(u), i1 = i0 + 1, f = u - i0; i0 < 0 -> += W, i1 >= W -> -= W (v alike with H);
    out = lerp(lerp(t00, t10, fu), lerp(t01, t11, fu), fv), lerp(a, b, t) = a + t * (b - a); non-finite uv -> 0.  float32 throughout."""
    assert filter_mode == "linear" and boundary_mode == "wrap" and not kw
    n, H, W, C = tex.shape
    u, v = uv[..., 0], uv[..., 1]
    finite = torch.isfinite(u) & torch.isfinite(v)
    u = torch.where(finite, u, torch.zeros_like(u))
    v = torch.where(finite, v, torch.zeros_like(v))
    u = u - torch.floor(u)
    v = v - torch.floor(v)
    u = u * float(W) - 0.5
    v = v * float(H) - 0.5
    fu0, fv0 = torch.floor(u), torch.floor(v)
    fu, fv = (u - fu0)[..., None], (v - fv0)[..., None]
    iu0, iv0 = fu0.long(), fv0.long()
    iu1, iv1 = iu0 + 1, iv0 + 1
    iu0 = torch.where(iu0 < 0, iu0 + W, iu0)
    iv0 = torch.where(iv0 < 0, iv0 + H, iv0)
    iu1 = torch.where(iu1 >= W, iu1 - W, iu1)
    iv1 = torch.where(iv1 >= H, iv1 - H, iv1)
    flat = tex.reshape(n, H * W, C)

    def tap(iy, ix):
        idx = (iy * W + ix).reshape(n, -1, 1).expand(-1, -1, C)
        return torch.gather(flat, 1, idx).reshape(iy.shape + (C,))
    lerp = lambda a, b, t: a + t * (b - a)
    out = lerp(lerp(tap(iv0, iu0), tap(iv0, iu1), fu), lerp(tap(iv1, iu0), tap(iv1, iu1), fu), fv)
    return torch.where(finite[..., None], out, torch.zeros_like(out))


def torchvision_gaussian_blur(img, kernel_size, sigma=None):
    """restates torchvision.transforms.functional.gaussian_blur for a float tensor [B, C, H, W] (functional.py + _functional_tensor.py)"""
    if isinstance(kernel_size, int):
        kernel_size = [kernel_size, kernel_size]
    for ksize in kernel_size:
        if ksize % 2 == 0 or ksize < 0:
            raise ValueError(f"kernel_size should have odd and positive integers. Got {kernel_size}")
    if sigma is None:
        sigma = [ksize * 0.15 + 0.35 for ksize in kernel_size]

    def k1d(ksize, s):
        ksize_half = (ksize - 1) * 0.5
        x = torch.linspace(-ksize_half, ksize_half, steps=ksize, dtype=img.dtype)
        pdf = torch.exp(-0.5 * (x / s).pow(2))
        return pdf / pdf.sum()
    kx, ky = k1d(kernel_size[0], sigma[0]), k1d(kernel_size[1], sigma[1])
    kernel = torch.mm(ky[:, None], kx[None, :]).expand(img.shape[-3], 1, kernel_size[1], kernel_size[0])
    padding = [kernel_size[0] // 2, kernel_size[0] // 2, kernel_size[1] // 2, kernel_size[1] // 2]
    x = torch.nn.functional.pad(img, padding, mode="reflect")
    return torch.nn.functional.conv2d(x, kernel, groups=img.shape[-3])


def install_variant_seams():
    dr = importlib.import_module("nvdiffrast.torch")
    dr.texture = nvdiffrast_texture_linear_wrap
    tvf = importlib.import_module("torchvision.transforms.functional")
    tvf.gaussian_blur = torchvision_gaussian_blur
    gb = importlib.import_module("TextureTools.texturetools.image.gaussian_blur")
    assert gb.gaussian_blur_tv is torchvision_gaussian_blur


# ---------------------------------------------------------------------------------------------------
def _views(HW, seed, fx, fy):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, HW), np.linspace(0, 1, HW), indexing="ij")
    imgs = np.zeros((6, HW, HW, 3), np.float32)
    for v in range(6):
        ph = rng.uniform(0, 6.28, 6)
        for c in range(3):
            imgs[v, ..., c] = 0.5 + 0.5 * np.sin(fx * xx + ph[c]) * np.cos(fy * yy + ph[c + 3])
    return imgs.astype(np.float16).astype(np.float32), xx, yy


def _cameras(radius, perspective):
    gen = importlib.import_module("TextureTools.texturetools.camera.generator")
    c2ws = gen.generate_box_views_c2ws(radius)[[0, 1, 4, 2, 3, 5]]
    if perspective:
        intr = gen.generate_intrinsics(FOV, FOV, fov=True, degree=True)
    else:
        intr = gen.generate_intrinsics(1.15, 1.15, fov=False, degree=False)      # the unit sphere spans ndc [-1.15, 1.15]: it crosses every border
    return c2ws, intr


def _uv(inv, c2ws, intr, imgs, alpha_fn, perspective, mode, HW, T):
    image_attrs = torch.from_numpy(imgs)
    mv = inv.mv_to_pcd(c2ws, intr, (HW, HW), image_attrs=image_attrs, perspective=perspective, filt_gradient_points=False)
    alpha = mv["alpha_visiable"].clone() * alpha_fn
    uv = inv.uv_to_pcd(c2ws, intr, (T, T), image_attrs=image_attrs, alpha_attrs=alpha, perspective=perspective, ray_normal_angle_threhold=100,
                       grid_interpolate_mode=mode)
    return mv, alpha, uv


def _bake(inv, uv, method, kb=3, kbb=3, kblur=5):
    bake = inv.bake_mv_to_uv_reproject_blur(uv["point_cloud_2d_visiable"], uv["point_cloud_2d"], uv["mask_2d_visiable"], uv["mask_2d"],
                                            method=method, kernel_size_boundary=kb, kernel_size_boundary_blur=kbb, kernel_size_blur=kblur)
    # the atlas after the seam blur, before pull-push, at the covered texels (point_cloud_2d.colors, :626)
    return bake["color_2d"].numpy().copy(), bake["point_cloud_2d"].colors.numpy().copy()


def g67g_gaussian(out):
    inv, R, (verts, faces, uvs) = _make_inverse_renderer()
    c2ws, intr = _cameras(2.8, True)
    HW, T = 48, 96
    imgs, xx, yy = _views(HW, 41, 7, 5)
    hole = torch.from_numpy((((xx - 0.5) ** 2 + (yy - 0.5) ** 2) > 0.16 ** 2) | (xx < 0.3)).float()[None, :, :, None]
    fix = dict(verts=verts, faces=faces, uvs=uvs, c2ws=c2ws.numpy(), intr=intr.numpy(), images=imgs.astype(np.float16))
    with torch.no_grad():
        mv, alpha, uv = _uv(inv, c2ws, intr, imgs, hole, True, "torch", HW, T)
        fix.update(alpha=np.packbits(alpha.numpy() > 0), mv_alpha=np.packbits(mv["alpha"].numpy() > 0), mask_2d=np.packbits(uv["mask_2d"].numpy()),
                   mask_2d_visiable=np.packbits(uv["mask_2d_visiable"].numpy()))
        seams = {}
        for tag, sizes in (("d", (3, 3, 5)), ("s", (5, 5, 7))):
            c_g, pre_g = _bake(inv, uv, "gaussian", *sizes)
            c_l, pre_l = _bake(inv, uv, "lens", *sizes)
            seams[tag] = np.any(pre_g != pre_l, -1)          # the texels the blur replaced (a subset of the seam mask)
            assert seams[tag].sum() > 50, "the Gaussian atlas must differ from the lens atlas on the seam"
            fix["color_2d_gauss_" + tag] = c_g
            if tag == "s":
                fix["pre_gauss_s"] = pre_g      # the blurred atlas before pull-push at the covered texels (one size: the file stays small)
            print("G67g %s %s: %d seam texels where the blurs differ" % (tag, sizes, int(seams[tag].sum())))
        assert not np.array_equal(seams["d"], seams["s"]), "the seam mask at 5 / 5 must differ from the one at 3 / 3"
    np.savez_compressed(os.path.join(out, "g67g_reproject_gaussian.npz"), **fix)


def g67n_nvdiff(out):
    inv, R, (verts, faces, uvs) = _make_inverse_renderer()
    HW, T = 48, 96
    imgs, xx, yy = _views(HW, 43, 6, 4)
    fix = dict(verts=verts, faces=faces, uvs=uvs, images=imgs.astype(np.float16))
    for tag, perspective, radius in (("o", False, 2.8), ("p", True, 1.8)):
        c2ws, intr = _cameras(radius, perspective)
        hole = torch.from_numpy(((xx - 0.5) ** 2 + (yy - 0.5) ** 2) > 0.16 ** 2).float()[None, :, :, None]      # no border strip: it would hide the wrap
        with torch.no_grad():
            mv, alpha, uv = _uv(inv, c2ws, intr, imgs, hole, perspective, "nvdiff", HW, T)
            _, _, uv_t = _uv(inv, c2ws, intr, imgs, hole, perspective, "torch", HW, T)
            diff = int((uv["mask_2d_visiable"] != uv_t["mask_2d_visiable"]).sum())
            print("G67n %s: %d texel-views differ between 'torch' and 'nvdiff'; visible per view %s" % (
                tag, diff, uv["mask_2d_visiable"].sum((1, 2, 3)).tolist()))
            assert diff >= 20, "the wrap boundary must change the visibility of at least 20 texel-views"
            c, _ = _bake(inv, uv, "lens")
        fix.update({"c2ws_" + tag: c2ws.numpy(), "intr_" + tag: intr.numpy(),
                    "alpha_" + tag: np.packbits(alpha.numpy() > 0), "mv_alpha_" + tag: np.packbits(mv["alpha"].numpy() > 0),
                    "mask_2d_" + tag: np.packbits(uv["mask_2d"].numpy()), "mask_2d_visiable_" + tag: np.packbits(uv["mask_2d_visiable"].numpy()),
                    "mask_2d_visiable_torch_" + tag: np.packbits(uv_t["mask_2d_visiable"].numpy()),
                    "color_2d_" + tag: c})
        if perspective:      # the per-view sampled colours of one set (the file stays small)
            fix["vis_colors_p"] = uv["point_cloud_2d_visiable"].colors.numpy()
    np.savez_compressed(os.path.join(out, "g67n_backprojection_nvdiff.npz"), **fix)


def main():
    sys.path.insert(0, REF)
    install_stubs()
    install_variant_seams()
    torch.set_num_threads(4)
    only = set(sys.argv[1:])
    for fn in (g67g_gaussian, g67n_nvdiff):
        if only and fn.__name__ not in only:
            continue
        fn(HERE)
        print("wrote", fn.__name__)


if __name__ == "__main__":
    main()
