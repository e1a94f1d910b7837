"""Image outpainting on the device: image/image_outpainting.py of the reference.

The reference quantises its float tensors to uint8, copies them to the host, resizes the mask with cv2.erode / cv2.dilate and calls cv2.inpaint with
cv2.INPAINT_NS (Navier-Stokes) [3p] per image.  INPAINT_NS is not built.  What is built is the same hand-off around this library's Telea inpainting
(ops.inpaint_telea, csrc/inpaint.hip, DESIGN 8 "Telea inpainting"), chosen by name with the keyword method='telea'; the default, method='ns', is the
reference's and is refused by name (NotImplementedError), never replaced silently.
"""
import torch

from . import ops
from .image_fusion import _quantise


def image_outpainting(src, mask, n_erode_pix=0, n_radius=1, method="ns"):
    """src [B,H,W,C] (1 <= C <= 4; the reference: 3), mask [B,H,W,1] float in [0, 1], broadcast against each other -> [B,H,W,C] in src's dtype: per image, on
    the quantised uint8 values (clamp(0, 1) * 255 truncated), the pixels under the mask (its last channel, non-zero; resized by n_erode_pix with
    ops.mask_morph: > 0 erodes, < 0 dilates) are filled from the others with radius n_radius, the pixels outside it are kept; the result / 255.
    method='telea': ops.inpaint_telea.  method='ns' (the default, the reference's cv2.INPAINT_NS): NotImplementedError naming 'telea'."""
    if method == "ns":
        raise NotImplementedError("image_outpainting(method='ns') is not built (cv2.inpaint, INPAINT_NS): pass method='telea' for the Telea fill")
    if method != "telea":
        raise ValueError("image_outpainting: method %r, expected 'telea' (built) or 'ns' (refused)" % (method,))
    if src.dim() != 4 or mask.dim() != 4:
        raise ValueError("image_outpainting: src [B, H, W, C] and mask [B, H, W, 1] are 4-dimensional")
    if not (src.is_cuda and mask.device == src.device and src.is_floating_point() and mask.is_floating_point()):
        raise ValueError("image_outpainting: src and mask are float tensors in [0, 1] on one CUDA device")
    B, H, W, _ = torch.broadcast_shapes(src.shape, mask.shape)
    src_e, mask_e = src.expand(B, H, W, -1), mask.expand(B, H, W, -1)
    res = torch.empty(src_e.shape, dtype=src.dtype, device=src.device)
    for i in range(B):
        m = ops.mask_morph(_quantise(mask_e[i, :, :, -1]).contiguous(), n_erode_pix)
        out = ops.inpaint_telea(_quantise(src_e[i]).contiguous(), m, radius=n_radius)[0]
        res[i] = out.to(src.dtype).div(255.0)
    return res
