"""Restatement (TEST INFRASTRUCTURE ONLY), written for this project, of the blended UV texture bake (utx_uv_bake with its epilogue, utx_uv_dilation_step and the
loop of ops.uv_dilation; the reference: texture/reprojection/mesh_remapping.py:145-270, :430-505, texture/reprojection/uv_dilation.py:33-50, :80-92) in numpy,
shared by tests/test_uv_bake_cpu.py and tests/test_uv_bake_gpu.py, with the counted bounds.  Every function evaluates in the kernel's operation order in
float32, so the GPU is held to it bit for bit; against the reference's own arrays (fixture G21) the bounds below hold.

Bounds (U = 2^-24; every bound is for the DIFFERENCE of two float32 evaluations that make the same vis / cov / threshold decisions):
  sample   the six channels of a view sampled bilinearly at uv: oracle.gbuffer_ref.map_bound('bilinear', ...) = (14 M + 4 (W + H) R) U per channel, the bound
           counted for G18's map_attr and used for G19's (M: the largest |texel|, R: the range of the map with the padding's zero).  uv itself is equal on
           both sides (G19 pins it bit for bit), hence so are vis, cov and uv_alpha, which are integer decisions on it.
  weight   w = ((k (c c) (c c)) a) (1 - e), a in {0, 1}: dw <= k (4 |c|^3 dc + c^4 de) + 12 U |w|   (6 roundings per side)
  colour   col = (a s + (1 - a) kd) w: a s and (1 - a) kd are exact (a is 0 or 1), so inner = s or kd; d col <= |w| ds + |inner| dw + 4 U |col|
  sums     B terms in ANY order (torch's .sum(0) may pair them): sum_b d col_b + 2 (B - 1) U sum_b |col_b|, and the same for w
  overlay  q = acc / w where w > conf: dq <= (d acc + |q| dw) / w + 2 U |q|
  soft     (kd (conf - w) + x) / conf: d <= (|kd| dw + dx + 8 U (|kd| conf + |x|)) / conf;   hard: 0
  dilation one step is a mean of at most nine valid taps, so it passes the largest input deviation of its window on and adds (9 + 3) roundings per side at
           the scale of the largest |colour|: after n steps d <= max d_in + 24 n U max|colour|; the clamp does not increase it.
  outpaint pull_push is a pyramid of weighted means and lerps (at most 14 roundings per level and side): d <= max d_in + 28 L U max|colour| with
           L = ceil(log2(T)) + 1 levels."""
import math
import os

import numpy as np

from . import uv_project_ref as UVP
from .gbuffer_ref import map_bound
from .pixel_ref import bake_epilogue

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
F32, F64, U = np.float32, np.float64, 2.0 ** -24
_FIX = {}


def g21():
    """the fixture, read once and shared (the arrays are never written to)"""
    if not _FIX:
        with np.load(os.path.join(GOLD, "g21_uv_bake.npz"), allow_pickle=False) as f:
            _FIX.update({k: f[k] for k in f.files})
        for v in _FIX.values():
            v.setflags(write=False)
    return _FIX


def g21_images():
    """[6,4,R,R] float32 = k / 255 as the maker formed them"""
    return g21()["images_u8"].astype(F32) / F32(255.0)


def g21_map_Kd():
    return g21()["map_Kd_u8"].astype(F32) / F32(255.0)


def g21_inputs(tag):
    """the arrays utx_uv_bake takes, from what the reference handed its own lookups: dict for uv_bake(**) above (B = 3, or 6 for tag '6')"""
    f = g21()
    B = f["face_mask_" + tag].shape[0]
    rast_view = np.zeros(f["cover_" + tag].shape + (4,), F32)
    rast_view[..., 3] = f["cover_" + tag]
    w = f["weights3"] if B == 3 else np.asarray([2.0, 0.05, 0.2, 1.0, 0.2, 0.05], F32)
    return dict(rast2d=f["rast2d"], faces=f["faces"], face_mask=f["face_mask_" + tag], v_ndc=f["v_ndc_" + tag], images=g21_images()[:B], wmap=f["wmap_" + tag],
                rast_view=rast_view, map_Kd=g21_map_Kd(), weights=w)


def six_channels(images, wmap):
    """images [B,4,R,R] planar, wmap [B,R,R,2] -> the [B,R,R,6] map of project_uv_texture (:480)"""
    return np.concatenate([np.transpose(np.asarray(images, F32), (0, 2, 3, 1)), np.asarray(wmap, F32)], -1)


def uv_bake(rast2d, faces, face_mask, v_ndc, images, wmap, rast_view, map_Kd, weights, use_alpha=True, detail=None):
    """utx_uv_bake in its operation order (float32) -> (acc [Th,Tw,4], wacc [Th,Tw,1]); detail (a dict) receives uv_alpha, cov, s (the six samples) per view"""
    m6 = six_channels(images, wmap)
    p = UVP.uv_project(rast2d, faces, face_mask, v_ndc, m6, rast_view, "bilinear", None)
    s, ua = p["map_attr"].astype(F32), p["uv_alpha"].astype(F32)
    B = s.shape[0]
    kd = np.asarray(map_Kd, F32)
    acc, wacc = np.zeros(kd.shape, F32), np.zeros(kd.shape[:2] + (1,), F32)
    one = F32(1.0)
    cols, ws = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            a = ua[b] if use_alpha else np.ones_like(ua[b])
            c, e = s[b, ..., 4:5], s[b, ..., 5:6]
            w = ((F32(weights[b]) * ((c * c) * (c * c))) * a) * (one - e)
            col = (a * s[b, ..., :4] + (one - a) * kd) * w
            acc, wacc = acc + col, wacc + w
            cols.append(col)
            ws.append(w)
    if detail is not None:
        detail.update(uv_alpha=ua, cov=p["cov"], s=s, col=np.stack(cols), w=np.stack(ws), uv=p["uv"])
    return acc.astype(F32), wacc.astype(F32)


def bake_bound(images, wmap, map_Kd, weights, use_alpha, detail):
    """(d acc [Th,Tw,4], d wacc [Th,Tw,1]): the module docstring's bound for the difference of two evaluations, per texel, in float64"""
    m6 = six_channels(images, wmap).astype(F64)
    s, ua = detail["s"].astype(F64), detail["uv_alpha"].astype(F64)
    kd = np.asarray(map_Kd, F64)
    B = s.shape[0]
    e_acc, e_w = np.zeros(kd.shape), np.zeros(kd.shape[:2] + (1,))
    m_acc, m_w = np.zeros(kd.shape), np.zeros(kd.shape[:2] + (1,))
    for b in range(B):
        mb = map_bound("bilinear", [m6[b]])
        # a texel off the view's coverage reads texel [0][0]: no sampling error there
        ds = np.where(detail["cov"][b][..., None], mb[None, None, :], 0.0)
        a = ua[b] if use_alpha else np.ones_like(ua[b])
        c, e = s[b, ..., 4:5], s[b, ..., 5:6]
        k = abs(float(weights[b]))
        w = k * c ** 4 * a * np.abs(1 - e)
        dw = a * k * (4 * np.abs(c) ** 3 * ds[..., 4:5] * np.abs(1 - e) + c ** 4 * ds[..., 5:6]) + 12 * U * w
        inner = a * s[b, ..., :4] + (1 - a) * kd
        col = np.abs(inner) * w
        e_acc += w * a * ds[..., :4] + np.abs(inner) * dw + 4 * U * col
        e_w += dw
        m_acc += col
        m_w += w
    return e_acc + 2 * (B - 1) * U * m_acc, e_w + 2 * (B - 1) * U * m_w


def epilogue(acc, wacc, map_Kd, rast2d, overlay_confidence, blending, blending_confidence, inpainting_confidence):
    """remapping_uv_texture :205-228 in float32 -> (overlay, blended [Th,Tw,4], inpaint mask uint8 [Th,Tw]); blending None | 'soft' | 'hard'.  The thresholds
    are float32 values: a float32 tensor is compared with a Python number in float32"""
    over, out = bake_epilogue(acc, wacc, map_Kd, overlay_confidence, blending, blending_confidence, F32)
    mask = (np.asarray(wacc, F32)[..., 0] <= F32(inpainting_confidence)) & (np.asarray(rast2d)[..., 3] > 0)
    return over, out, mask.astype(np.uint8)


def epilogue_bound(acc, wacc, map_Kd, e_acc, e_w, overlay_confidence, blending, blending_confidence):
    """d blended [Th,Tw,4] for two evaluations that fall on the same side of every threshold"""
    acc, wacc, kd = np.asarray(acc, F64), np.asarray(wacc, F64), np.asarray(map_Kd, F64)
    oc, bc = float(F32(overlay_confidence)), float(F32(blending_confidence))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = acc / wacc
        dq = (e_acc + np.abs(q) * e_w) / wacc + 2 * U * np.abs(q)
    hi = wacc > oc
    x, dx = np.where(hi, q, acc), np.where(hi, dq, e_acc)
    if blending == "soft":
        ds = (np.abs(kd) * e_w + dx + 8 * U * (np.abs(kd) * bc + np.abs(x))) / bc
        dx = np.where(wacc <= bc, ds, dx)
    elif blending == "hard":
        dx = np.where(wacc <= bc, 0.0, dx)
    return dx


def dilation_step(col, mask):
    """utx_uv_dilation_step (UTX_UVD_STEP) in its operation order: col [H,W,C] float32, mask [H,W] (non-zero = valid) -> (col, mask uint8, invalid left)"""
    col, m = np.asarray(col, F32), np.asarray(mask) != 0
    H, W, C = col.shape
    nine = F32(9.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pre = np.where(m[..., None], col, col * F32(0.0))
        pc = np.zeros((H + 2, W + 2, C), F32)
        pm = np.zeros((H + 2, W + 2), F32)
        inside = np.zeros((H + 2, W + 2), bool)
        pc[1:-1, 1:-1], pm[1:-1, 1:-1], inside[1:-1, 1:-1] = pre, m.astype(F32), True
        S, M = np.zeros((H, W, C), F32), np.zeros((H, W), F32)
        for k in range(9):
            dy, dx = k // 3, k % 3
            t, tm, ins = pc[dy:dy + H, dx:dx + W], pm[dy:dy + H, dx:dx + W], inside[dy:dy + H, dx:dx + W]
            S = np.where(ins[..., None], S + t, S)      # a tap outside the image is not visited
            M = np.where(ins, M + tm, M)
        md = M / nine
        boundary = (md - m.astype(F32)) != 0
        out = np.where(boundary[..., None], (S / nine) / md[..., None], col)
    mo = M > 0
    return out.astype(F32), mo.astype(np.uint8), int((~mo).sum())


def clamp01(col):
    col = np.asarray(col, F32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(col), col, np.minimum(np.maximum(col, F32(0.0)), F32(1.0))).astype(F32)


def uv_dilation(col, valid, max_iters=-1, trace=None):
    """ops.uv_dilation: the loop, its three stops and the closing clamp -> (col [H,W,C], steps)"""
    cur, mask = np.asarray(col, F32), (np.asarray(valid) != 0).astype(np.uint8)
    steps, count = 0, int((mask == 0).sum())
    while count > 0 and not (max_iters > 0 and steps >= max_iters):
        cur, mask, now = dilation_step(cur, mask)
        steps += 1
        if trace is not None:
            trace.append((cur, mask))
        if now >= count:
            break
        count = now
    return clamp01(cur), steps


def dilation_bound(d_in, steps, cmax):
    return d_in + 24.0 * steps * U * cmax


def outpaint_bound(d_in, T, cmax):
    return d_in + 28.0 * (math.ceil(math.log2(max(T, 2))) + 1) * U * cmax


def torch_reference_step(col, mask):
    """one step as the reference forms it, from torch's own avg_pool2d on the CPU (count_include_pad, divisor 9): col [H,W,C], mask [H,W] bool ->
    (col [H,W,C], mask bool); the colour must already be premultiplied by the mask"""
    import torch
    c = torch.from_numpy(np.ascontiguousarray(np.transpose(np.asarray(col, F32), (2, 0, 1))))[None]
    m = torch.from_numpy(np.asarray(mask) != 0)[None, None].to(torch.float32)
    md = torch.nn.functional.avg_pool2d(m, 3, 1, 1)
    cd = torch.nn.functional.avg_pool2d(c, 3, 1, 1)
    out = torch.where(torch.abs(md - m).to(torch.bool), cd / md, c)
    return out[0].permute(1, 2, 0).numpy(), md[0, 0].to(torch.bool).numpy()


def torch_reference_dilation(col, valid, max_iters=-1, give_up=64):
    """uv_dilation.py:40-49 around torch_reference_step; give_up bounds the loop where the reference would not end -> (col, steps)"""
    import torch
    col = np.asarray(col, F32)
    m = np.asarray(valid) != 0
    with np.errstate(invalid="ignore"):
        cur = col * m[..., None].astype(F32)
    cnt = 0
    while not (m.all() or (max_iters > 0 and cnt >= max_iters) or cnt >= give_up):
        cur, m = torch_reference_step(cur, m)
        cnt += 1
    mf = m[..., None].astype(F32)
    with np.errstate(invalid="ignore"):
        out = torch.clamp(torch.from_numpy(mf * cur + (F32(1.0) - mf) * col), 0.0, 1.0).numpy()
    return out, cnt


# ---- small synthetic scenes for the GPU tests: a fan of triangles in the atlas, views that are plain 2-D maps of the vertices
def synthetic_scene(Th, Tw, B, R, seed, off_coverage=False):
    """dict of float32 / int32 / uint8 arrays for utx_uv_bake: the atlas raster is made BY HAND (no rasteriser): texel (y, x) lies on triangle (x + y) % F with
    barycentrics from a fixed pattern, some texels uncovered; v_ndc spreads the vertices over and a little past [-1, 1]; rast_view covers a disc (or,
    off_coverage, leaves holes where visible texels land); face_mask hides some faces per view."""
    rng = np.random.default_rng(seed)
    V, F = 7, 5
    faces = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [1, 6, 2]], np.int32)
    yy, xx = np.meshgrid(np.arange(Th), np.arange(Tw), indexing="ij")
    u = rng.uniform(0.0, 1.0, (Th, Tw)).astype(F32)
    v = (rng.uniform(0.0, 1.0, (Th, Tw)) * (1.0 - u)).astype(F32)
    tri = ((xx + 2 * yy) % (F + 1)).astype(F32)      # 0 = uncovered
    rast2d = np.stack([u, v, np.zeros_like(u), tri], -1).astype(F32)
    rast2d[tri == 0, :2] = 0.0
    v_ndc = rng.uniform(-1.15, 1.15, (B, V, 2)).astype(F32)
    face_mask = (rng.uniform(0, 1, (B, F)) < 0.75).astype(np.uint8)
    face_mask[:, 0] = 1
    images = rng.uniform(-0.25, 1.25, (B, 4, R, R)).astype(F32)
    wmap = np.stack([rng.uniform(-1.0, 0.0, (B, R, R)), (rng.uniform(0, 1, (B, R, R)) < 0.3).astype(np.float64)], -1).astype(F32)
    rast_view = np.zeros((B, R, R, 4), F32)
    rast_view[..., 3] = (rng.uniform(0, 1, (B, R, R)) < (0.5 if off_coverage else 0.9)).astype(F32) * rng.integers(1, F + 1, (B, R, R))
    map_Kd = rng.uniform(0.0, 1.0, (Th, Tw, 4)).astype(F32)
    weights = rng.uniform(0.05, 2.0, B).astype(F32)
    return dict(rast2d=rast2d, faces=faces, face_mask=face_mask, v_ndc=v_ndc, images=images, wmap=wmap, rast_view=rast_view, map_Kd=map_Kd, weights=weights)
