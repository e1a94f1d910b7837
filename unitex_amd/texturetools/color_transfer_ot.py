"""Sliced optimal-transport colour transfer on the device: image/color_transfer_ot.py of the reference (D. Coeurjolly's OTColorTransfer in @iperov's port).

The reference runs steps x batch_size numpy argsorts over the whole image on the host and regularises with OpenCV's cv2.bilateralFilter [3p].  Here the loop
(ops.color_transfer_ot: projection, rocPRIM radix sorts, scatter, update) and the filter (ops.bilateral_filter) stay on the device; the host only draws the
steps x batch_size directions, exactly as the reference draws them, and uploads them once.  The loop is the reference's bit for bit wherever no two projections
of a batch are equal (tests/golden/g26_color_transfer_ot.npz); ties, which numpy's argsort leaves open, go to the smaller pixel index.  The filter's rule is this
library's on OpenCV's documented parameters and is not pinned against OpenCV.  DESIGN 8 "Colour transfer".

It harmonises the colours of two bakes, or of a view and an atlas, before image_fusion blends them."""
import numpy as np
import torch

from . import ops


def draw_directions(steps, batch_size, C):
    """float32 [steps * batch_size, C]: per step and batch np.random.normal(size=(C,)).astype(float32) divided by its float32 norm, from numpy's GLOBAL
    generator in the reference's order -- a caller who seeds numpy gets the reference's directions"""
    dirs = np.empty((steps * batch_size, C), np.float32)
    for k in range(steps * batch_size):
        d = np.random.normal(size=(C,)).astype(np.float32)
        dirs[k] = d / np.linalg.norm(d, axis=-1)
    return dirs


def CTSOT(src, dst, steps=10, batch_size=5, reg_sigmaXY=16.0, reg_sigmaV=5.0, dirs=None):
    """Color Transform via Sliced Optimal Transfer.

    src, dst     CUDA float32 [H, W, C] of one shape, any range, 1 <= C <= 4
    steps        number of solver steps
    batch_size   directions per step
    reg_sigmaXY  the regulariser's spatial sigma; 0.0: no regularisation.  Otherwise src + bilateral_filter(new - src, reg_sigmaV, reg_sigmaXY), C 1 or 3
    reg_sigmaV   the regulariser's colour sigma
    dirs         the unit directions, [steps * batch_size, C] (numpy or tensor); None: draw_directions from numpy's global generator

    Nothing is clipped, as in the reference.  Non-finite pixels are not checked: a check would cost a read-back, and the loop has none."""
    who = "CTSOT"
    if not (isinstance(src, torch.Tensor) and isinstance(dst, torch.Tensor)) or src.dim() != 3 or tuple(src.shape) != tuple(dst.shape):
        raise ValueError("%s: src and dst are expected as tensors [H, W, C] of one shape" % who)
    steps, batch_size = int(steps), int(batch_size)
    if steps < 0 or batch_size < 1:
        raise ValueError("%s: steps is %d and batch_size %d, expected steps >= 0 and batch_size >= 1" % (who, steps, batch_size))
    C = src.shape[2]
    if not 1 <= C <= 4:
        raise ValueError("%s: %d channels, 1 .. 4 are built" % (who, C))
    reg = float(reg_sigmaXY) != 0.0
    if reg and C not in (1, 3):
        raise ValueError("%s: regularisation (reg_sigmaXY != 0) of %d channels: the bilateral filter takes 1 or 3, pass reg_sigmaXY=0.0" % (who, C))
    if not (src.is_cuda and dst.device == src.device and src.dtype == torch.float32 and dst.dtype == torch.float32):
        raise ValueError("%s: src and dst are expected as float32 on one CUDA device" % who)
    if dirs is None:
        dirs = draw_directions(steps, batch_size, C)
    if not isinstance(dirs, torch.Tensor):
        dirs = torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float32))
    dirs = dirs.to(device=src.device, dtype=torch.float32)
    new = ops.color_transfer_ot(src, dst, dirs, steps, batch_size)
    if reg:
        new = src + ops.bilateral_filter(new - src, reg_sigmaV, reg_sigmaXY)
    return new
