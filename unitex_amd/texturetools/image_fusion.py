"""Poisson image fusion (seamless clone) on the device: image/image_fusion.py of the reference.

The reference quantises its float tensors to uint8, copies them to the host and calls OpenCV's seamlessClone(NORMAL_CLONE) [3p] per image.  Here the
quantisation, the mask resize, the right-hand side, the solve (multigrid V-cycles, csrc/image_fusion.hip) and the rounding stay on the device; the one host
round trip is the 16-byte bounding rectangle per image, which sizes the solver's levels.  The fusion rule is this library's, written out in DESIGN 8
"Poisson image fusion"; where it follows OpenCV's choices (the 3-fold 3 x 3 erosion, the tight bounding rectangle, the source zeroed outside the mask) it is
not pinned against OpenCV, which is not available to the tests.

Built: image_fusion, image_fusion_hybrid.  Refused by name (NotImplementedError): color_transfer=True (an HSV histogram transfer through cv2.cvtColor; it is
NOT the sliced optimal-transport transfer of color_transfer_ot.CTSOT, which is built and may be run on src before the fusion),
smooth_fusion and the boundary_color_shift experiments (beside cv2.inpaint, which ops.inpaint_telea now covers, cv2 contours, scipy interpolators and k-d trees), image_soft_fusion
(a 175-tap cv2.GaussianBlur).

The blended UV bake's 'poisson' branch (mesh_remapping.py:213) runs in remapping_uv.remapping_uv_texture_cv (remapping_uv_texture keeps refusing it) as the composition:
    acc, wacc = project_uv_texture(mesh, c2ws, intrinsics, images, map_Kd, weights)
    overlay = torch.where(wacc > overlay_confidence, acc / wacc, acc)
    rgb = image_fusion(overlay[None, ..., :3], map_Kd[None, ..., :3], (wacc > blending_confidence).float()[None])[0]
"""
import torch

from . import ops


def _quantise(t):
    """the reference's hand-off: clamp(0, 1) * 255 truncated to uint8"""
    return t.clamp(0.0, 1.0).mul(255).to(torch.uint8)


def _expand(name, src, dst, mask, *more):
    if src.dim() != 4 or dst.dim() != 4 or mask.dim() != 4 or any(m.dim() != 4 for m in more):
        raise ValueError("%s: src, dst [B, H, W, 3] and the masks [B, H, W, 1] are 4-dimensional" % name)
    if not (src.is_cuda and dst.device == src.device and mask.device == src.device and all(m.device == src.device for m in more)):
        raise ValueError("%s: src, dst and the masks live on one CUDA device" % name)
    if not (src.is_floating_point() and dst.is_floating_point() and mask.is_floating_point() and all(m.is_floating_point() for m in more)):
        raise ValueError("%s: float tensors in [0, 1] are expected" % name)
    B, H, W, _ = torch.broadcast_shapes(src.shape, dst.shape, mask.shape)      # the reference leaves mask_boundary out of the shape as well
    if src.shape[-1] != 3 or dst.shape[-1] != 3:
        raise ValueError("%s: src and dst have 3 channels" % name)
    return B, [t.expand(B, H, W, -1) for t in (src, dst, mask) + more]


def image_fusion(src, dst, mask, n_erode_pix=0, color_transfer=False):
    """src [B,H,W,3], dst [B,H,W,3], mask [B,H,W,1] float in [0, 1], broadcast against each other -> [B,H,W,3] in src's dtype: src blended into dst under the
    mask (its last channel, resized by n_erode_pix) in the gradient domain, per image, on the quantised uint8 values; the result / 255."""
    if color_transfer:
        raise NotImplementedError("image_fusion(color_transfer=True) is not built: the HSV histogram transfer (transfer_skin_color_np, cv2.cvtColor)")
    B, (src_e, dst_e, mask_e) = _expand("image_fusion", src, dst, mask)
    res = torch.empty(src_e.shape, dtype=src.dtype, device=src.device)
    for i in range(B):
        out = ops.image_fusion_u8(_quantise(src_e[i]).contiguous(), _quantise(dst_e[i]).contiguous(), _quantise(mask_e[i, :, :, -1]).contiguous(),
                                  n_erode_pix=n_erode_pix)
        res[i] = out.to(src.dtype).div(255.0)
    return res


def image_fusion_hybrid(src, dst, mask, mask_boundary, n_erode_pix=0):
    """image_fusion with dst blended hard towards src along mask_boundary first (image_fusion_hybrid_np): on the uint8 values, with the mask resized by n_erode_pix,
    mb = mask_boundary where mask > 127, else 0;  dst' = uint8(clip((src m + dst (1 - m)) b + dst (1 - b), 0, 255)) with m = mask / 255, b = mb / 255 in
    float64, truncated; then the fusion of src into dst' under the resized mask."""
    B, (src_e, dst_e, mask_e, mb_e) = _expand("image_fusion_hybrid", src, dst, mask, mask_boundary)
    res = torch.empty(src_e.shape, dtype=src.dtype, device=src.device)
    for i in range(B):
        s, d = _quantise(src_e[i]).contiguous(), _quantise(dst_e[i]).contiguous()
        m = ops.mask_morph(_quantise(mask_e[i, :, :, -1]).contiguous(), n_erode_pix)
        mb = _quantise(mb_e[i, :, :, -1]) * (m > 127).to(torch.uint8)
        sf, df = s.to(torch.float64), d.to(torch.float64)
        mf, bf = (m.to(torch.float64) / 255.0)[..., None], (mb.to(torch.float64) / 255.0)[..., None]
        d2 = ((sf * mf + df * (1.0 - mf)) * bf + df * (1.0 - bf)).clamp(0.0, 255.0).to(torch.uint8)
        res[i] = ops.image_fusion_u8(s, d2.contiguous(), m).to(src.dtype).div(255.0)
    return res


def _refused(name, why):
    def f(*args, **kwargs):
        raise NotImplementedError("%s is not built: %s" % (name, why))
    f.__name__ = name
    f.__doc__ = "%s of the reference: refused, %s" % (name, why)
    return f


image_soft_fusion = _refused("image_soft_fusion", "cv2.GaussianBlur over a 175 x 175 window")
smooth_fusion = _refused("smooth_fusion", "cv2.inpaint between the fusions")
boundary_color_shift = _refused("boundary_color_shift", "cv2.findContours / cv2.inpaint")
boundary_color_shift_v2 = _refused("boundary_color_shift_v2", "scipy's LinearNDInterpolator on the host")
boundary_color_shift_v3 = _refused("boundary_color_shift_v3", "scipy's KDTree on the host")
boundary_color_shift_v4 = _refused("boundary_color_shift_v4", "an experiment at a fixed 128 x 128 size")
boundary_color_shift_v5 = _refused("boundary_color_shift_v5", "cv2.findContours and scipy's KDTree")
boundary_color_shift_v6 = _refused("boundary_color_shift_v6", "cv2.findContours")
