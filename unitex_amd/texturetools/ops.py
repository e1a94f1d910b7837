"""Functional wrappers over the geometry half of the C ABI (tensor in / tensor out, all on the GPU).
Used by the parity tests and by NVDiffRendererInverse / VideoExporter."""
import ctypes as C
import math

import numpy as np
import torch

from .._lib import BackprojectDesc, ptr
from ..flux.ops import get_ctx

F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def _f(t):
    assert t.is_cuda and t.dtype == F32 and t.is_contiguous(), "expected a contiguous CUDA float32 tensor"
    return t


def _i(t):
    assert t.is_cuda and t.dtype == I32 and t.is_contiguous(), "expected a contiguous CUDA int32 tensor"
    return t


def _opt(t):
    """the pointer of an optional float32 tensor"""
    return ptr(_f(t)) if t is not None else None


def transform_points(verts, mvp, want_ndc=True):
    """verts [V,3], mvp [n,4,4] -> clip [n,V,4], ndc [n,V,2]"""
    ctx = get_ctx(verts.device.index)
    V, n = verts.shape[0], mvp.shape[0]
    clip = torch.empty(n, V, 4, dtype=F32, device=verts.device)
    ndc = torch.empty(n, V, 2, dtype=F32, device=verts.device) if want_ndc else None
    ctx.check(ctx.lib.utx_transform_points(ctx.handle, ptr(_f(verts)), V, ptr(_f(mvp)), n, ptr(clip), ptr(ndc), ctx.stream()))
    return clip, ndc


def rasterize(pos_clip, tri, H, W):
    """pos_clip [V,4], tri [F,3] int32 -> rast [H,W,4] = (u, v, z/w, id+1)"""
    ctx = get_ctx(pos_clip.device.index)
    F = tri.shape[0]
    rast = torch.empty(H, W, 4, dtype=F32, device=pos_clip.device)
    wb = ctx.lib.utx_rasterize_workspace_bytes(F, H, W)
    work = torch.empty(wb, dtype=U8, device=pos_clip.device)
    ctx.check(ctx.lib.utx_rasterize(ctx.handle, ptr(_f(pos_clip)), ptr(_i(tri)), F, H, W, ptr(rast), ptr(work), ctx.stream()))
    return rast


def chart_flood(adj, bucket):
    """adj [F,3] int32 (face across each edge, -1 = border), bucket [F] int32 -> chart [F] int32: smallest face index of the
    connected same-bucket component (utx_chart_flood; synchronises the stream)."""
    ctx = get_ctx(adj.device.index)
    F = adj.shape[0]
    chart = torch.empty(F, dtype=torch.int32, device=adj.device)
    flag = torch.zeros(1, dtype=torch.int32, device=adj.device)
    rc = ctx.lib.utx_chart_flood(ctx.handle, ptr(_i(adj)), ptr(_i(bucket)), F, ptr(chart), ptr(flag), ctx.stream())
    if rc < 0:
        ctx.check(rc)
    return chart


def interpolate(attr, rast, tri):
    ctx = get_ctx(attr.device.index)
    H, W = rast.shape[:2]
    Cc = attr.shape[1]
    out = torch.empty(H, W, Cc, dtype=F32, device=attr.device)
    ctx.check(ctx.lib.utx_interpolate(ctx.handle, ptr(_f(attr)), Cc, ptr(_f(rast)), ptr(_i(tri)), H * W, ptr(out), ctx.stream()))
    return out


def condition_shade(rast, nrm, pos, bg):
    """rast [N,H,W,4], nrm/pos [N,H,W,3] -> uint8 normal, ccm [N,H,W,3], alpha [N,H,W]"""
    ctx = get_ctx(rast.device.index)
    npix = rast.numel() // 4
    on = torch.empty(rast.shape[:-1] + (3,), dtype=U8, device=rast.device)
    oc = torch.empty_like(on)
    oa = torch.empty(rast.shape[:-1], dtype=U8, device=rast.device)
    arr = (C.c_float * 3)(*[float(x) for x in bg])
    ctx.check(ctx.lib.utx_condition_shade(ctx.handle, ptr(_f(rast)), ptr(_f(nrm)), ptr(_f(pos)), arr, npix, ptr(on), ptr(oc), ptr(oa), ctx.stream()))
    return on, oc, oa


def face_normals(verts, faces):
    ctx = get_ctx(verts.device.index)
    out = torch.empty(faces.shape[0], 3, dtype=F32, device=verts.device)
    ctx.check(ctx.lib.utx_face_normals(ctx.handle, ptr(_f(verts)), ptr(_i(faces)), faces.shape[0], ptr(out), ctx.stream()))
    return out


def texture_shade(rast, uv01, tri, tex, bg=(1.0, 1.0, 1.0)):
    """rast [H,W,4], uv01 [V,2], tex [Ht,Wt,3] fp32 (UV-raster orientation) -> uint8 RGB [H,W,3]."""
    ctx = get_ctx(rast.device.index)
    H, W = rast.shape[:2]
    out = torch.empty(H, W, 3, dtype=U8, device=rast.device)
    bgv = (C.c_float * 3)(*[float(b) for b in bg])
    ctx.check(ctx.lib.utx_texture_shade(ctx.handle, ptr(_f(rast)), ptr(_f(uv01)), ptr(_i(tri)), ptr(_f(tex)), tex.shape[0], tex.shape[1],
                                        bgv, H * W, ptr(out), ctx.stream()))
    return out


GBUFFER_MODES = {"world_normal": 0, "camera_normal": 1, "world_position": 2, "camera_position": 3, "z_depth": 4, "distance": 5}


def _gbuffer_attr(mode, attr):
    """per-vertex attribute [V,C] (a view of a wider contiguous tensor is fine: e.g. clip[..., 3:] or cam[..., :3] of transform_points)
    -> (tensor, stride in floats); C = 1 for z_depth, 3 otherwise."""
    m = GBUFFER_MODES[mode]
    assert attr.is_cuda and attr.dtype == F32 and attr.dim() == 2 and attr.shape[1] == (1 if m == 4 else 3)
    assert attr.shape[1] == 1 or attr.stride(1) == 1, "the channels of a vertex must be adjacent"
    return m, attr, int(attr.stride(0))


def gbuffer_shade(mode, rast, tri, attr, scale2=None, ndc=False, bg=(1.0, 1.0, 1.0), want_rgba=False):
    """rast [H,W,4], per-vertex attr of `mode` (see utx_gbuffer_shade) -> uint8 RGB [H,W,3] (, float RGBA [H,W,4]).
    scale2: CUDA float32 [2] = (lo, hi) to normalise the covered pixels with, or None; bg=None skips the composite."""
    ctx = get_ctx(rast.device.index)
    H, W = rast.shape[:2]
    m, attr, stride = _gbuffer_attr(mode, attr)
    out = torch.empty(H, W, 3, dtype=U8, device=rast.device)
    rgba = torch.empty(H, W, 4, dtype=F32, device=rast.device) if want_rgba else None
    flags = (1 if ndc else 0) | (2 if bg is not None else 0)
    bgv = (C.c_float * 3)(*[float(b) for b in (bg if bg is not None else (0.0, 0.0, 0.0))])
    ctx.check(ctx.lib.utx_gbuffer_shade(ctx.handle, m, ptr(_f(rast)), ptr(_i(tri)), ptr(attr), stride, ptr(_f(scale2) if scale2 is not None else None),
                                        flags, bgv, H * W, ptr(out), ptr(rgba), ctx.stream()))
    return (out, rgba) if want_rgba else out


def gbuffer_range(mode, rast, tri, attr, out=None):
    """(lo, hi) of the mode's buffer over the covered pixels of this frame, and the 'covers nothing' flag, both left on the device:
    returns a CUDA float32 [3] whose [:2] is the scale2 of gbuffer_shade and whose [2], viewed as int32, is 1 if the frame is empty."""
    ctx = get_ctx(rast.device.index)
    m, attr, stride = _gbuffer_attr(mode, attr)
    out = torch.empty(3, dtype=F32, device=rast.device) if out is None else out
    ctx.check(ctx.lib.utx_gbuffer_range(ctx.handle, m, ptr(_f(rast)), ptr(_i(tri)), ptr(attr), stride, rast.shape[0] * rast.shape[1],
                                        ptr(out), C.c_void_p(out.data_ptr() + 8), ctx.stream()))
    return out


def camera_normals(nrm, c2ws):
    """nrm [V,3], c2ws [n,4,4] -> [n,V,3] = normalize(nrm @ c2ws[:, :3, :3]) per vertex."""
    ctx = get_ctx(nrm.device.index)
    V, n = nrm.shape[0], c2ws.shape[0]
    out = torch.empty(n, V, 3, dtype=F32, device=nrm.device)
    ctx.check(ctx.lib.utx_camera_normals(ctx.handle, ptr(_f(nrm)), V, ptr(_f(c2ws)), n, ptr(out), ctx.stream()))
    return out


def _camera_arrays(v_pos, v_nrm, c2ws, B, need_pos, need_nrm, v_pos_cam, v_nrm_cam):
    """(v_pos_cam, v_nrm_cam) [B,V,3] of uv_gbuffer / screen_gbuffer: each is built from c2ws [B,4,4] with the existing kernels (transform_points
    with M = w2c, camera_normals) only when a requested buffer reads it, the caller did not pass it, and there is a view (B > 0)"""
    if B > 0 and need_pos and v_pos_cam is None:
        from . import camera
        w2c = camera.c2w_to_w2c(torch.as_tensor(c2ws, dtype=F32).cpu()).to(v_pos.device, F32).contiguous()
        v_pos_cam = transform_points(v_pos, w2c, want_ndc=False)[0][..., :3].contiguous()
    if B > 0 and need_nrm and v_nrm_cam is None:
        assert v_nrm is not None, "v_nrm [V, 3] is required by the normal buffers"
        v_nrm_cam = camera_normals(v_nrm, torch.as_tensor(c2ws, dtype=F32).to(v_pos.device).contiguous())
    return v_pos_cam, v_nrm_cam


def _background(who, background, dev):
    """`background` of screen_gbuffer / uv_project -> (bg_kind of the ABI, the scalar, expand): None, a number, a [C] vector or a dense image.
    expand(shape, of="") is what the kernel reads for a buffer of shape (B, H, W, C): the vector or the image made contiguous, None for the other kinds."""
    if background is None or isinstance(background, (int, float)):
        return (0 if background is None else 1), float(background or 0.0), lambda shape, of="": None
    if not isinstance(background, torch.Tensor):
        raise ValueError("%s: background is %r: expected None, a number or a tensor" % (who, type(background)))
    bgt = background.to(dev, F32)
    kind = 2 if bgt.dim() <= 1 else 3

    def expand(shape, of=""):
        try:
            return bgt.expand(shape[-1] if kind == 2 else shape).contiguous()
        except RuntimeError:
            raise ValueError("%s: background %s does not broadcast to %s%s" % (who, tuple(bgt.shape), tuple(shape), of))
    return kind, 0.0, expand


# name -> (bit of utx_uv_gbuffer's `want`, channels, one layer per camera); the order is the header's UTX_UVGB_* bits
UV_GBUFFERS = {"mask": (0, 1, False), "alpha": (1, 1, False), "world_normal": (2, 3, False), "world_position": (3, 3, False),
               "camera_normal": (4, 3, True), "camera_position": (5, 3, True), "distance": (6, 1, True), "z_depth": (7, 1, True),
               "ray_direction": (8, 3, True), "cos_ray_normal": (9, 1, True)}
UV_GBUFFERS_POS_CAM = ("camera_position", "distance", "z_depth", "ray_direction", "cos_ray_normal")      # read v_pos_cam
UV_GBUFFERS_NRM_CAM = ("camera_normal", "cos_ray_normal")                                                # read v_nrm_cam


def uv_gbuffer(rast2d, faces, v_pos, v_nrm, c2ws=None, want=("mask", "alpha", "world_normal", "world_position"), v_pos_cam=None, v_nrm_cam=None):
    """The atlas-space geometry buffers of simple_inverse_rendering in one launch (utx_uv_gbuffer): rast2d [H2D,W2D,4] (the UV raster), faces [F,3]
    int32, v_pos / v_nrm [V,3] (v_nrm may be None when no normal buffer is requested), c2ws [B,4,4] or None -> dict of the buffers named in
    `want` (UV_GBUFFERS): mask uint8 [H2D,W2D], alpha [H2D,W2D,1], world_* [1,H2D,W2D,3], the camera-dependent ones [B,H2D,W2D,C].  The per-view per-vertex arrays are built here with the existing kernels
    (transform_points with M = w2c, camera_normals), as the reference builds them in front of dr.interpolate; a caller that holds them already
    (e.g. the reference's own, in the parity tests) passes v_pos_cam / v_nrm_cam [B,V,3] and c2ws is then not read."""
    want = tuple(want)
    for k in want:
        if k not in UV_GBUFFERS:
            raise KeyError("uv_gbuffer: unknown buffer %r (known: %s)" % (k, ", ".join(UV_GBUFFERS)))
    if not want:
        raise ValueError("uv_gbuffer: no buffer requested")
    need_pos, need_nrm = any(k in UV_GBUFFERS_POS_CAM for k in want), any(k in UV_GBUFFERS_NRM_CAM for k in want)
    if (need_pos and v_pos_cam is None or need_nrm and v_nrm_cam is None) and c2ws is None:
        raise ValueError("uv_gbuffer: %s depend on the cameras: c2ws is required" % ", ".join(k for k in want if UV_GBUFFERS[k][2]))
    ctx = get_ctx(rast2d.device.index)
    dev = rast2d.device
    H, W = rast2d.shape[:2]
    V = v_pos.shape[0]
    n_cams = torch.as_tensor(c2ws).shape[0] if c2ws is not None else 0
    v_pos_cam, v_nrm_cam = _camera_arrays(v_pos, v_nrm, c2ws, n_cams, need_pos, need_nrm, v_pos_cam, v_nrm_cam)
    per_view = [a for a in (v_pos_cam, v_nrm_cam) if a is not None]
    B = per_view[0].shape[0] if per_view else n_cams
    for a in per_view:
        assert tuple(a.shape) == (B, V, 3), "per-view vertex arrays are [B, V, 3]"
    assert faces.shape[1] == 3 and rast2d.shape[2] == 4 and tuple(v_pos.shape) == (V, 3)
    if "world_normal" in want or (need_nrm and v_nrm_cam is None):
        assert v_nrm is not None and tuple(v_nrm.shape) == (V, 3), "v_nrm [V, 3] is required by the normal buffers"
    out, bits = {}, 0
    ptrs = (C.c_void_p * len(UV_GBUFFERS))()
    for k in want:
        bit, ch, per = UV_GBUFFERS[k]
        if k == "mask":
            out[k] = torch.empty(H, W, dtype=U8, device=dev)
        elif k == "alpha":
            out[k] = torch.empty(H, W, 1, dtype=F32, device=dev)
        else:
            out[k] = torch.empty(B if per else 1, H, W, ch, dtype=F32, device=dev)
        ptrs[bit] = out[k].data_ptr() or None
        bits |= 1 << bit
    if B == 0:      # no camera: the camera-dependent buffers are empty, and an empty tensor has no address to hand over
        bits &= ~sum(1 << UV_GBUFFERS[k][0] for k in want if UV_GBUFFERS[k][2])
        if bits == 0:
            return out
    ctx.check(ctx.lib.utx_uv_gbuffer(ctx.handle, ptr(_f(rast2d)), ptr(_i(faces)), ptr(_f(v_pos)), _opt(v_nrm), _opt(v_pos_cam if B else None),
                                     _opt(v_nrm_cam if B else None), V, B, H, W, bits, ptrs, ctx.stream()))
    return out


# name -> (bit of utx_screen_gbuffer's `want`, channels; None: the caller's); the order is the header's UTX_SGB_* bits
SCREEN_GBUFFERS = {"mask": (0, 1), "alpha": (1, 1), "world_normal": (2, 3), "camera_normal": (3, 3), "world_position": (4, 3), "camera_position": (5, 3),
                   "distance": (6, 1), "ray_direction": (7, 3), "z_depth": (8, 1), "cos_ray_normal": (9, 1), "v_attr": (10, None), "uv": (11, 2),
                   "map_attr": (12, None)}
SCREEN_GBUFFERS_POS_CAM = ("camera_position", "distance", "ray_direction", "cos_ray_normal")      # read v_pos_cam
SCREEN_GBUFFERS_NRM_CAM = ("camera_normal", "cos_ray_normal")                                     # read v_nrm_cam
SCREEN_FILTERS = {"bilinear": 0, "nearest": 1, "nvdiffrast": 2}                                   # UTX_SGB_FILTER_*
SCREEN_MAX_MAPS = 4                                                                               # UTX_SGB_MAX_MAPS


def screen_gbuffer(rast, faces, v_pos, v_nrm=None, v_uv=None, v_attr=None, maps=(), mvp=None, c2ws=None, want=("mask", "alpha"), background=None,
                   filter="bilinear", clip_w=None, v_pos_cam=None, v_nrm_cam=None):
    """The screen-space buffers of simple_rendering in one launch (utx_screen_gbuffer): rast [B,H,W,4] (one utx_rasterize per view), faces [F,3]
    int32, v_pos [V,3], and whatever the requested buffers read: v_nrm [V,3], v_uv [V,2] in [-1,1], v_attr [V,Ca], maps = up to four [Ht,Wt,C]
    tensors of their own sizes, mvp [B,4,4] (z_depth: clip w) and c2ws [B,4,4] (the camera-space buffers) -> dict of the buffers named in `want`
    (SCREEN_GBUFFERS): mask uint8 [B,H,W], every other one float32 [B,H,W,C].  background (v_attr and map_attr only): None, a number, or a tensor
    that broadcasts to [B,H,W,C]; filter: 'bilinear' | 'nearest' (grid_sample, zero padding, align_corners=False) | 'nvdiffrast' (linear, wrap).
    The per-view per-vertex arrays are built here with the existing kernels only when a requested buffer reads them (transform_points with M = mvp
    and M = w2c, camera_normals), as the reference builds them in front of dr.interpolate; a caller that holds them already passes clip_w [B,V],
    v_pos_cam / v_nrm_cam [B,V,3], and mvp / c2ws are then not read."""
    want = tuple(want)
    for k in want:
        if k not in SCREEN_GBUFFERS:
            raise KeyError("screen_gbuffer: unknown buffer %r (known: %s)" % (k, ", ".join(SCREEN_GBUFFERS)))
    if not want:
        raise ValueError("screen_gbuffer: no buffer requested")
    if filter not in SCREEN_FILTERS:
        raise ValueError("screen_gbuffer: filter %r (known: %s)" % (filter, ", ".join(SCREEN_FILTERS)))
    need_pos, need_nrm = any(k in SCREEN_GBUFFERS_POS_CAM for k in want), any(k in SCREEN_GBUFFERS_NRM_CAM for k in want)
    need_w = "z_depth" in want
    if (need_pos and v_pos_cam is None or need_nrm and v_nrm_cam is None) and c2ws is None:
        raise ValueError("screen_gbuffer: %s depend on the cameras: c2ws is required" % ", ".join(k for k in want if k in SCREEN_GBUFFERS_POS_CAM + SCREEN_GBUFFERS_NRM_CAM))
    if need_w and clip_w is None and mvp is None:
        raise ValueError("screen_gbuffer: z_depth is the interpolated clip w: mvp (or clip_w) is required")
    assert rast.dim() == 4 and rast.shape[3] == 4 and faces.shape[1] == 3, "rast is [B, H, W, 4], faces [F, 3]"
    ctx = get_ctx(rast.device.index)
    dev = rast.device
    B, H, W = rast.shape[:3]
    V = v_pos.shape[0]
    assert tuple(v_pos.shape) == (V, 3)
    if B > 0:
        if need_w and clip_w is None:
            clip_w = transform_points(v_pos, torch.as_tensor(mvp, dtype=F32).to(dev).contiguous(), want_ndc=False)[0][..., 3].contiguous()
        v_pos_cam, v_nrm_cam = _camera_arrays(v_pos, v_nrm, c2ws, B, need_pos, need_nrm, v_pos_cam, v_nrm_cam)
        for a, shp in ((clip_w, (B, V)), (v_pos_cam, (B, V, 3)), (v_nrm_cam, (B, V, 3))):
            if a is not None and tuple(a.shape) != shp:
                raise ValueError("screen_gbuffer: a per-view vertex array is %s, expected %s" % (tuple(a.shape), shp))
    if "world_normal" in want and (v_nrm is None or tuple(v_nrm.shape) != (V, 3)):
        raise ValueError("screen_gbuffer: world_normal reads v_nrm [V, 3]")
    if ("uv" in want or "map_attr" in want) and (v_uv is None or tuple(v_uv.shape) != (V, 2)):
        raise ValueError("screen_gbuffer: uv and map_attr read v_uv [V, 2]")
    Ca = Cm = 0
    if "v_attr" in want:
        if v_attr is None or v_attr.dim() != 2 or v_attr.shape[0] != V or v_attr.shape[1] < 1:
            raise ValueError("screen_gbuffer: v_attr is %s, expected [V = %d, Ca >= 1]" % (None if v_attr is None else tuple(v_attr.shape), V))
        Ca = v_attr.shape[1]
    maps = tuple(maps) if "map_attr" in want else ()
    if "map_attr" in want:
        if not 1 <= len(maps) <= SCREEN_MAX_MAPS:
            raise ValueError("screen_gbuffer: map_attr samples 1 to %d maps, got %d" % (SCREEN_MAX_MAPS, len(maps)))
        for m in maps:
            if m.dim() != 3 or min(m.shape) < 1:
                raise ValueError("screen_gbuffer: a map is %s, expected [Ht, Wt, C] with no empty side" % (tuple(m.shape),))
        Cm = sum(m.shape[2] for m in maps)
    # the background: None, a number, a [C] vector or a dense image, per buffer (the two channel counts may differ)
    kind, scalar, expand = _background("screen_gbuffer", background if "v_attr" in want or "map_attr" in want else None, dev)
    bgs = {k: expand((B, H, W, ch), " of " + k) if k in want else None for k, ch in (("v_attr", Ca), ("map_attr", Cm))}
    out, bits = {}, 0
    ptrs = (C.c_void_p * len(SCREEN_GBUFFERS))()
    for k in want:
        bit, ch = SCREEN_GBUFFERS[k]
        ch = {"v_attr": Ca, "map_attr": Cm}.get(k, ch)
        out[k] = torch.empty(B, H, W, dtype=U8, device=dev) if k == "mask" else torch.empty(B, H, W, ch, dtype=F32, device=dev)
        ptrs[bit] = out[k].data_ptr() or None
        bits |= 1 << bit
    if B * H * W == 0:      # nothing to write, and an empty tensor has no address to hand over
        return out
    mptr = (C.c_void_p * SCREEN_MAX_MAPS)(*[_f(m).data_ptr() for m in maps])
    mdim = (C.c_int * (3 * SCREEN_MAX_MAPS))(*[int(d) for m in maps for d in m.shape])
    ctx.check(ctx.lib.utx_screen_gbuffer(ctx.handle, ptr(_f(rast)), ptr(_i(faces)), ptr(_f(v_pos)), _opt(v_nrm), _opt(v_uv), _opt(v_attr if Ca else None), Ca,
                                         _opt(clip_w), _opt(v_pos_cam), _opt(v_nrm_cam), V, B, H, W, len(maps), mptr, mdim, SCREEN_FILTERS[filter], kind, scalar,
                                         _opt(bgs["v_attr"]), _opt(bgs["map_attr"]), bits, ptrs, ctx.stream()))
    return out


def _u8(t):
    assert t.is_cuda and t.dtype == U8 and t.is_contiguous(), "expected a contiguous CUDA uint8 tensor"
    return t


def visible_faces_rays(bvh, c2ws, perspective=True, force_stack=False, face_order=False, count=False):
    """utx_visible_faces_rays: Mesh.get_visible_faces of the reference on the tree `bvh` (ops.BVH): c2ws [B,4,4] -> mask uint8 [B,F].  One ray per
    (view, face) aimed at the face's centroid marks the face it hits first (closest hit, t >= 0, ties to the smallest id, no backface culling).
    force_stack: the stack walk instead of the packed one (equal masks); face_order: rays in face order instead of the tree's sorted leaf order
    (equal masks); count: also return the number of tree nodes the rays visited."""
    c2ws = _f(c2ws)
    if c2ws.dim() != 3 or tuple(c2ws.shape[1:]) != (4, 4) or c2ws.shape[0] < 1:
        raise ValueError("visible_faces_rays: c2ws is %s, expected [B >= 1, 4, 4]" % (tuple(c2ws.shape),))
    ctx = bvh.ctx
    B, F = c2ws.shape[0], bvh.faces.shape[0]
    mask = torch.empty(B, F, dtype=U8, device=c2ws.device)
    visited = torch.zeros(1, dtype=torch.int64, device=c2ws.device) if count else None
    ctx.check(ctx.lib.utx_visible_faces_rays(ctx.handle, bvh.handle, ptr(bvh.verts), ptr(bvh.faces), F, ptr(c2ws), B, int(bool(perspective)),
                                             (1 if force_stack else 0) | (2 if face_order else 0), ptr(mask), ptr(visited) if count else None, ctx.stream()))
    return (mask, int(visited.item())) if count else mask


def visible_faces_raster(rast, F):
    """utx_visible_faces_raster: rast [B,H,W,4] -> mask uint8 [B,F] of the faces whose id appears in a view's raster (renderer_base.py:77-81)"""
    assert rast.dim() == 4 and rast.shape[3] == 4, "rast is [B, H, W, 4]"
    ctx = get_ctx(rast.device.index)
    B, H, W = rast.shape[:3]
    mask = torch.empty(B, int(F), dtype=U8, device=rast.device)
    ctx.check(ctx.lib.utx_visible_faces_raster(ctx.handle, ptr(_f(rast)), B, H, W, int(F), ptr(mask), ctx.stream()))
    return mask


def erode_faces(mask, faces, V, depth=1):
    """utx_erode_faces: erode_face of the reference (topology.py:12-25) on every row of mask uint8 [B,F]: `depth` times, a face stays set iff none of
    its vertices belongs to an unset face.  Returns a new mask."""
    assert mask.dim() == 2 and mask.shape[1] == faces.shape[0], "mask is [B, F]"
    out = _u8(mask).clone()
    if depth <= 0:
        return out
    ctx = get_ctx(mask.device.index)
    B, F = mask.shape
    vstamp = torch.empty(B, int(V), dtype=I32, device=mask.device)
    ctx.check(ctx.lib.utx_erode_faces(ctx.handle, ptr(out), ptr(_i(faces)), B, F, int(V), int(depth), ptr(vstamp), ctx.stream()))
    return out


def visible_vertices(mask, faces, V):
    """utx_visible_vertices: mask uint8 [B,F] -> uint8 [B,V]: a vertex is set iff it belongs to a set face"""
    assert mask.dim() == 2 and mask.shape[1] == faces.shape[0], "mask is [B, F]"
    ctx = get_ctx(mask.device.index)
    B, F = mask.shape
    out = torch.empty(B, int(V), dtype=U8, device=mask.device)
    ctx.check(ctx.lib.utx_visible_vertices(ctx.handle, ptr(_u8(mask)), ptr(_i(faces)), B, F, int(V), ptr(out), ctx.stream()))
    return out


def uv_project(rast2d, faces, face_mask, v_ndc, map_attr=None, rast_map=None, filter="bilinear", background=None):
    """utx_uv_project, the atlas-space view projection in one launch: rast2d [H,W,4] (the atlas raster), faces [F,3] int32, face_mask uint8 [B,F]
    (visible_faces_*), v_ndc [B,V,2] (transform_points) -> dict: 'uv' [B,H,W,2] (the view's NDC of the texel's surface point, -1 where the view does not
    see it) and 'uv_alpha' [B,H,W,1]; with map_attr [Bm,Hm,Wm,C] (Bm = 1 or B) and rast_map [B,Hm,Wm,4] (the views rasterised at the map's size) also
    'map_attr' [B,H,W,C], and uv_alpha additionally needs the view's coverage at uv.  filter: SCREEN_FILTERS; background: None (texels without coverage
    take the map's texel [0, 0]), a number, or a tensor that broadcasts to [B,H,W,C] (it fills the texels with uv_alpha = 0)."""
    if filter not in SCREEN_FILTERS:
        raise ValueError("uv_project: filter %r (known: %s)" % (filter, ", ".join(SCREEN_FILTERS)))
    assert rast2d.dim() == 3 and rast2d.shape[2] == 4 and faces.shape[1] == 3, "rast2d is [H, W, 4], faces [F, 3]"
    H, W = rast2d.shape[:2]
    F = faces.shape[0]
    if face_mask.dim() != 2 or face_mask.shape[1] != F or face_mask.shape[0] < 1:
        raise ValueError("uv_project: face_mask is %s, expected [B >= 1, F = %d]" % (tuple(face_mask.shape), F))
    B = face_mask.shape[0]
    if v_ndc.dim() != 3 or v_ndc.shape[0] != B or v_ndc.shape[2] != 2:
        raise ValueError("uv_project: v_ndc is %s, expected [B = %d, V, 2]" % (tuple(v_ndc.shape), B))
    V = v_ndc.shape[1]
    dev = rast2d.device
    Bm = Hm = Wm = Cm = kind = 0
    scalar, bg = 0.0, None
    if map_attr is not None:
        if map_attr.dim() != 4 or min(map_attr.shape) < 1 or map_attr.shape[0] not in (1, B):
            raise ValueError("uv_project: map_attr is %s, expected [1 or B = %d, Hm, Wm, C] with no empty side" % (tuple(map_attr.shape), B))
        Bm, Hm, Wm, Cm = map_attr.shape
        if rast_map is None or tuple(rast_map.shape) != (B, Hm, Wm, 4):
            raise ValueError("uv_project: rast_map is %s, expected the views' rasters at the map's size %s" %
                             (None if rast_map is None else tuple(rast_map.shape), (B, Hm, Wm, 4)))
        kind, scalar, expand = _background("uv_project", background, dev)
        bg = expand((B, H, W, Cm))
    ctx = get_ctx(dev.index)
    out = {"uv_alpha": torch.empty(B, H, W, 1, dtype=F32, device=dev), "uv": torch.empty(B, H, W, 2, dtype=F32, device=dev)}
    if map_attr is not None:
        out["map_attr"] = torch.empty(B, H, W, Cm, dtype=F32, device=dev)
    if H * W == 0:
        return out
    ctx.check(ctx.lib.utx_uv_project(ctx.handle, ptr(_f(rast2d)), ptr(_i(faces)), F, ptr(_u8(face_mask)), ptr(_f(v_ndc)), V, B, H, W, _opt(map_attr), Bm, Hm, Wm, Cm,
                                     _opt(rast_map), SCREEN_FILTERS[filter], kind, scalar, _opt(bg), ptr(out["uv"]), ptr(out["uv_alpha"]),
                                     ptr(out["map_attr"]) if map_attr is not None else None, ctx.stream()))
    return out


def cubemap_tables(N, costheta_cutoff=None, device="cuda"):
    """utx_cubemap_table: (texels [6,N,N,4] = unit direction + pixel_area, tiles [6,nt,nt,4] or None) on `device`, built on the host in fp64.
    Runs without a GPU when device is 'cpu' (the tests' oracle reads the same table)."""
    from .._lib import load_library
    lib = load_library()
    tex = np.empty((6, N, N, 4), np.float32)
    nt = (N + 15) // 16
    tiles = np.empty((6, nt, nt, 4), np.float32) if costheta_cutoff is not None else None
    rc = lib.utx_cubemap_table(int(N), float(costheta_cutoff if costheta_cutoff is not None else 1.0), tex.ctypes.data_as(C.c_void_p),
                               tiles.ctypes.data_as(C.c_void_p) if tiles is not None else None)
    if rc != 0:
        raise ValueError("utx_cubemap_table(N=%d) -> %d: N must be even, 2 <= N <= 8192" % (N, rc))
    return torch.from_numpy(tex).to(device), (torch.from_numpy(tiles).to(device) if tiles is not None else None)


def latlong_to_cubemap(latlong, N):
    """latlong [Hi,Wi,3] -> cubemap [6,N,N,3] (utx_latlong_to_cubemap)"""
    ctx = get_ctx(latlong.device.index)
    out = torch.empty(6, N, N, 3, dtype=F32, device=latlong.device)
    ctx.check(ctx.lib.utx_latlong_to_cubemap(ctx.handle, ptr(_f(latlong)), latlong.shape[0], latlong.shape[1], N, ptr(out), ctx.stream()))
    return out


def cubemap_diffuse(cube, texels=None):
    """cube [6,N,N,3] -> the cosine-convolved cubemap (utx_cubemap_diffuse); texels: cubemap_tables(N)[0], built if None"""
    ctx = get_ctx(cube.device.index)
    N = cube.shape[1]
    assert cube.shape == (6, N, N, 3)
    if texels is None:
        texels, _ = cubemap_tables(N, None, cube.device)
    out = torch.empty_like(cube)
    ctx.check(ctx.lib.utx_cubemap_diffuse(ctx.handle, ptr(_f(cube)), N, ptr(_f(texels)), ptr(out), ctx.stream()))
    return out


def cubemap_specular(cube, roughness, costheta_cutoff, texels=None, tiles=None):
    """cube [6,N,N,3] -> the GGX-prefiltered cubemap over the lobe L.V >= costheta_cutoff (utx_cubemap_specular)"""
    ctx = get_ctx(cube.device.index)
    N = cube.shape[1]
    assert cube.shape == (6, N, N, 3)
    if texels is None or tiles is None:
        texels, tiles = cubemap_tables(N, costheta_cutoff, cube.device)
    out = torch.empty_like(cube)
    ctx.check(ctx.lib.utx_cubemap_specular(ctx.handle, ptr(_f(cube)), N, ptr(_f(texels)), ptr(_f(tiles)), float(roughness), float(costheta_cutoff), ptr(out),
                                           ctx.stream()))
    return out


def dfg_lut(R=256, n_samples=1024, device="cuda"):
    """split-sum table [R,R,2] (utx_dfg_lut), indexed (x = cos, y = roughness)"""
    device = torch.device(device if device != "cuda" else "cuda:%d" % torch.cuda.current_device())
    ctx = get_ctx(device.index)
    out = torch.empty(R, R, 2, dtype=F32, device=device)
    ctx.check(ctx.lib.utx_dfg_lut(ctx.handle, R, n_samples, ptr(out), ctx.stream()))
    return out


def cube_sample(cube, dirs):
    """cube [6,N,N,3], dirs [...,3] -> [...,3] by the library's cube lookup rule (include/unitex_hip.h)"""
    ctx = get_ctx(cube.device.index)
    d = _f(dirs.reshape(-1, 3))
    out = torch.empty_like(d)
    ctx.check(ctx.lib.utx_cube_sample(ctx.handle, ptr(_f(cube)), cube.shape[1], ptr(d), d.shape[0], ptr(out), ctx.stream()))
    return out.reshape(dirs.shape)


def scene_render(c2ws, intrinsics, H, W, cubemap=None, latlong=None, want=("rays_d",)):
    """cameras c2ws [B,4,4], intrinsics [3,3] or [B,3,3] looking into cubemap [6,N,N,C] / latlong [Hi,Wi,C] (utx_scene_render) -> a dict with the
    requested ones of rays_d [B,H,W,3], cubemap_attr [B,H,W,C], uv [B,H,W,2], latlong_map_attr [B,H,W,C], all from one launch"""
    ctx = get_ctx(c2ws.device.index)
    B, dev = c2ws.shape[0], c2ws.device
    unknown = set(want) - {"rays_d", "cubemap_attr", "uv", "latlong_map_attr"}
    if unknown or not want:
        raise ValueError("scene_render: want must name some of rays_d, cubemap_attr, uv, latlong_map_attr, got %r" % (tuple(want),))
    if "cubemap_attr" in want and cubemap is None:
        raise ValueError("scene_render: cubemap_attr needs a cubemap")
    if "latlong_map_attr" in want and latlong is None:
        raise ValueError("scene_render: latlong_map_attr needs a lat-long map")
    assert c2ws.shape == (B, 4, 4) and intrinsics.shape in ((3, 3), (B, 3, 3))
    Cs = {int(m.shape[-1]) for m, k in ((cubemap, "cubemap_attr"), (latlong, "latlong_map_attr")) if k in want}
    if len(Cs) > 1:
        raise ValueError("scene_render: the cubemap and the lat-long map must have the same number of channels")
    Cc = Cs.pop() if Cs else 3
    if cubemap is not None:
        assert cubemap.ndim == 4 and cubemap.shape[0] == 6 and cubemap.shape[1] == cubemap.shape[2]
    shapes = {"rays_d": 3, "cubemap_attr": Cc, "uv": 2, "latlong_map_attr": Cc}
    out = {k: torch.empty(B, H, W, shapes[k], dtype=F32, device=dev) for k in shapes if k in want}
    ctx.check(ctx.lib.utx_scene_render(ctx.handle, ptr(_f(c2ws)), ptr(_f(intrinsics)), 9 if intrinsics.ndim == 3 else 0, B, H, W, _opt(cubemap),
                                       cubemap.shape[1] if cubemap is not None else 0, _opt(latlong), latlong.shape[0] if latlong is not None else 0,
                                       latlong.shape[1] if latlong is not None else 0, Cc, ptr(out.get("rays_d")), ptr(out.get("cubemap_attr")), ptr(out.get("uv")),
                                       ptr(out.get("latlong_map_attr")), ctx.stream()))
    return out


def cubemap_to_latlong(cubemap, Ht, Wt):
    """cubemap [6,N,N,C] -> panorama [Ht,Wt,C] (utx_cubemap_to_latlong)"""
    ctx = get_ctx(cubemap.device.index)
    assert cubemap.ndim == 4 and cubemap.shape[0] == 6 and cubemap.shape[1] == cubemap.shape[2]
    out = torch.empty(Ht, Wt, cubemap.shape[3], dtype=F32, device=cubemap.device)
    ctx.check(ctx.lib.utx_cubemap_to_latlong(ctx.handle, ptr(_f(cubemap)), cubemap.shape[1], cubemap.shape[3], Ht, Wt, ptr(out), ctx.stream()))
    return out


def scene_bake_latlong(w2cs, projections, Ht, Wt, images=None):
    """M views (w2cs, projections [M,4,4]; images [M,H,W,C] or None) into one panorama (utx_scene_bake_latlong)
    -> (uv [M,Ht,Wt,2], uv_alpha [M,Ht,Wt,1], latlong_map_attr [Ht,Wt,C] or None without images)"""
    ctx = get_ctx(w2cs.device.index)
    M, dev = w2cs.shape[0], w2cs.device
    assert w2cs.shape == (M, 4, 4) and projections.shape == (M, 4, 4) and (images is None or (images.ndim == 4 and images.shape[0] == M))
    uv = torch.empty(M, Ht, Wt, 2, dtype=F32, device=dev)
    alpha = torch.empty(M, Ht, Wt, 1, dtype=F32, device=dev)
    H, W, Cc = (images.shape[1], images.shape[2], images.shape[3]) if images is not None else (0, 0, 0)
    out = torch.empty(Ht, Wt, Cc, dtype=F32, device=dev) if images is not None else None
    ctx.check(ctx.lib.utx_scene_bake_latlong(ctx.handle, ptr(_f(w2cs)), ptr(_f(projections)), _opt(images), M, H, W, Cc, Ht, Wt, ptr(uv), ptr(alpha), ptr(out),
                                             ctx.stream()))
    return uv, alpha, out


def pbr_forward(view_pos, world_pos, world_nrm, kd, ks, light_diffuse, light_specular, fg_lut):
    """dense PBRModel.forward (utx_pbr_forward): view_pos [3] or [npix,3], world_pos / world_nrm [npix,3], kd [npix,>=3], ks [npix,3]
    -> (diffuse, specular) [npix,3]"""
    ctx = get_ctx(world_pos.device.index)
    npix = world_pos.shape[0]
    d = torch.empty(npix, 3, dtype=F32, device=world_pos.device)
    s = torch.empty_like(d)
    ctx.check(ctx.lib.utx_pbr_forward(ctx.handle, ptr(_f(view_pos)), 0 if view_pos.numel() == 3 else 3, ptr(_f(world_pos)), ptr(_f(world_nrm)), ptr(_f(kd)),
                                      kd.shape[1], ptr(_f(ks)), ptr(_f(light_diffuse)), light_diffuse.shape[1], ptr(_f(light_specular)),
                                      light_specular.shape[1], ptr(_f(fg_lut)), fg_lut.shape[0], npix, ptr(d), ptr(s), ctx.stream()))
    return d, s


def pbr_shading_normal(view_pos, world_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm):
    """the shading normal of a tangent-space normal map (utx_pbr_shading_normal: bsdf_prepare_shading_normal, two-sided, OpenGL convention): view_pos [3] or
    [npix,3], the rest [npix,3] (perturbed_nrm = the decoded map value) -> [npix,3], not normalised"""
    ctx = get_ctx(world_pos.device.index)
    npix = world_pos.shape[0]
    out = torch.empty(npix, 3, dtype=F32, device=world_pos.device)
    ctx.check(ctx.lib.utx_pbr_shading_normal(ctx.handle, ptr(_f(view_pos)), 0 if view_pos.numel() == 3 else 3, ptr(_f(world_pos)), ptr(_f(perturbed_nrm)),
                                             ptr(_f(smooth_nrm)), ptr(_f(smooth_tng)), ptr(_f(geom_nrm)), npix, ptr(out), ctx.stream()))
    return out


def pbr_shade(rast, tri, v_pos, v_nrm, v_uv, kd, ks, eye, light_diffuse, light_specular, fg_lut, lambda_diffuse=1.0, lambda_specular=1.0,
              bg=(1.0, 1.0, 1.0), want_rgba=False, v_tng=None, f_nrm=None, normal_map=None):
    """one PBR frame (utx_pbr_shade): rast [H,W,4], kd [Hk,Wk,3] / ks [Hs,Ws,3] or None in UV-raster orientation, eye = 3 floats
    -> uint8 RGB [H,W,3] (, float RGBA [H,W,4]).
    v_tng [V,3] (meshes.vertex_tangents), f_nrm [F,3] (face_normals) and normal_map [Hn,Wn,3] (fp32, UV-raster orientation), all three or none: the frame is
    shaded with the map's normal (utx_pbr_shade_nm)."""
    nm_args = (v_tng, f_nrm, normal_map)
    if any(a is not None for a in nm_args) and any(a is None for a in nm_args):
        raise ValueError("pbr_shade: v_tng, f_nrm and normal_map go together (all three or none)")
    ctx = get_ctx(rast.device.index)
    H, W = rast.shape[:2]
    out = torch.empty(H, W, 3, dtype=U8, device=rast.device)
    rgba = torch.empty(H, W, 4, dtype=F32, device=rast.device) if want_rgba else None
    ev = (C.c_float * 3)(*[float(e) for e in eye])
    bgv = (C.c_float * 3)(*[float(b) for b in bg])
    ksp, Hs, Ws = ptr(_f(ks) if ks is not None else None), ks.shape[0] if ks is not None else 0, ks.shape[1] if ks is not None else 0
    lights = (ptr(_f(light_diffuse)), light_diffuse.shape[1], ptr(_f(light_specular)), light_specular.shape[1], ptr(_f(fg_lut)), fg_lut.shape[0],
              float(lambda_diffuse), float(lambda_specular), bgv, H * W, ptr(out), ptr(rgba), ctx.stream())
    if normal_map is None:
        ctx.check(ctx.lib.utx_pbr_shade(ctx.handle, ptr(_f(rast)), ptr(_i(tri)), ptr(_f(v_pos)), ptr(_f(v_nrm)), ptr(_f(v_uv)), ptr(_f(kd)), kd.shape[0], kd.shape[1],
                                        ksp, Hs, Ws, ev, *lights))
    else:
        assert v_tng.shape == v_nrm.shape and f_nrm.shape == tri.shape and normal_map.dim() == 3 and normal_map.shape[2] == 3
        ctx.check(ctx.lib.utx_pbr_shade_nm(ctx.handle, ptr(_f(rast)), ptr(_i(tri)), ptr(_f(v_pos)), ptr(_f(v_nrm)), ptr(_f(v_tng)), ptr(_f(f_nrm)), ptr(_f(v_uv)),
                                           ptr(_f(kd)), kd.shape[0], kd.shape[1], ksp, Hs, Ws, ptr(_f(normal_map)), normal_map.shape[0], normal_map.shape[1], ev,
                                           *lights))
    return (out, rgba) if want_rgba else out


INTERSECT_OUTPUTS = ("tid", "t", "loc", "uv", "front")


class BVH:
    """utx_bvh handle (RayTracing / APRMISRayTracing of the reference)."""

    def __init__(self, verts, faces):
        self.ctx = get_ctx(verts.device.index)
        self.verts, self.faces = _f(verts), _i(faces)   # kept alive: the handle borrows them
        h = C.c_void_p()
        # every array of the tree in ONE torch allocation (caching allocator: no hipMalloc / hipFree on the path), the build itself enqueued without a host wait (the wait moved one launch later: the first launch that needs the tree's depth blocks on the build's event once per tree)
        nbytes = int(self.ctx.lib.utx_bvh_workspace_bytes(faces.shape[0]))
        self.work = torch.empty(nbytes + 256, dtype=torch.uint8, device=verts.device)
        base = (self.work.data_ptr() + 255) & ~255
        self.ctx.check(self.ctx.lib.utx_bvh_build_ws(self.ctx.handle, ptr(self.verts), verts.shape[0], ptr(self.faces), faces.shape[0],
                                                     C.c_void_p(base), C.c_size_t(nbytes), C.byref(h), self.ctx.stream()))
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.ctx.lib.utx_bvh_free(self.handle)      # the handle only: the arrays are self.work, which torch releases stream-ordered like any other tensor
                self.handle = None
        except Exception:
            pass

    def arrays(self):
        """copies of (info [2F-1,3], aabb [2F-1,6], sorted codes [F], sorted ids [F]) as torch tensors"""
        a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        F = self.ctx.lib.utx_bvh_arrays(self.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        torch.cuda.synchronize()
        dev = self.verts.device

        def view(p, n, dtype):
            t = torch.empty(n, dtype=dtype, device=dev)
            import ctypes
            hip = ctypes.CDLL("libamdhip64.so")
            hip.hipMemcpy(ctypes.c_void_p(t.data_ptr()), p, ctypes.c_size_t(n * t.element_size()), 3)
            return t
        info = view(a, (2 * F - 1) * 3, I32).view(-1, 3)
        aabb = view(b, (2 * F - 1) * 6, F32).view(-1, 6)
        codes = view(c, F, I32)
        idx = view(d, F, I32)
        return info, aabb, codes, idx

    def trace(self, rays_o, rays_d):
        ro, rd = _f(rays_o.reshape(-1, 3)), _f(rays_d.reshape(-1, 3))
        tid = torch.empty(ro.shape[0], dtype=I32, device=ro.device)
        self.ctx.check(self.ctx.lib.utx_bvh_trace(self.ctx.handle, self.handle, ptr(ro), ptr(rd), ro.shape[0], ptr(tid), self.ctx.stream()))
        return tid

    def trace_count(self, rays_o, rays_d):
        """(tid, number of tree nodes the rays visited in total) -- the measurement behind bench.py's nodes_visited_per_ray"""
        ro, rd = _f(rays_o.reshape(-1, 3)), _f(rays_d.reshape(-1, 3))
        tid = torch.empty(ro.shape[0], dtype=I32, device=ro.device)
        visited = torch.zeros(1, dtype=torch.int64, device=ro.device)
        self.ctx.check(self.ctx.lib.utx_bvh_trace_count(self.ctx.handle, self.handle, ptr(ro), ptr(rd), ro.shape[0], ptr(tid), ptr(visited),
                                                        self.ctx.stream()))
        return tid, int(visited.item())

    def depth(self):
        """longest root-to-leaf path of the tree (<= 60: the stackless packed traversal is in use)"""
        return int(self.ctx.lib.utx_bvh_depth(self.handle))

    # ---- ray queries (csrc/raycast.hip): closest hit with every output, occlusion of segments, enclosed points
    def _rows(self, what, x, tail=(3,)):
        """x as a contiguous float32 [..., *tail] tensor on the tree's device, or a named ValueError"""
        if not torch.is_tensor(x) or not x.is_floating_point():
            raise ValueError("%s must be a floating-point tensor, got %s" % (what, x.dtype if torch.is_tensor(x) else type(x).__name__))
        if x.dim() != 1 + len(tail) or tuple(x.shape[1:]) != tuple(tail):
            raise ValueError("%s is %s, expected [N, %s]" % (what, tuple(x.shape), ", ".join(str(t) for t in tail)))
        if x.device != self.verts.device:
            raise ValueError("%s is on %s, the tree on %s" % (what, x.device, self.verts.device))
        if not x.shape[0] < 2 ** 31:
            raise ValueError("%s has %d rows, at most 2^31 - 1 are taken" % (what, x.shape[0]))
        return _f(x.to(F32).contiguous())

    def intersect(self, rays_o, rays_d, want=INTERSECT_OUTPUTS, force_stack=False, count=False, face_mask=None):
        """utx_bvh_intersect: the closest hit of the rays rays_o, rays_d [R,3] f32 (directions not normalised: t in units of |d|) -> dict of the buffers named in
        `want`: tid [R] i32 (-1: miss), t [R] f32 (+inf: miss), loc [R,3] = o + t d, uv [R,2] (Moeller-Trumbore's u, v of the winner), front [R] u8
        (dot(d, (v1 - v0) x (v2 - v0)) < 0).  The smallest t >= 0 wins, both sides count, ties to the smallest face id: the hit of visible_faces_rays, not the
        quirk-preserving id of trace().  A miss has loc = uv = front = 0.  face_mask [F] u8: the hit faces are set to 1 in it (not cleared).  count: also the
        number of tree nodes visited."""
        ro, rd = self._rows("intersect: rays_o", rays_o), self._rows("intersect: rays_d", rays_d)
        if ro.shape != rd.shape:
            raise ValueError("intersect: rays_o is %s, rays_d %s" % (tuple(ro.shape), tuple(rd.shape)))
        want = tuple(want)
        for k in want:
            if k not in INTERSECT_OUTPUTS:
                raise ValueError("intersect: unknown output %r (one of %s)" % (k, ", ".join(INTERSECT_OUTPUTS)))
        if face_mask is not None and (face_mask.dtype != torch.uint8 or tuple(face_mask.shape) != (self.faces.shape[0],) or not face_mask.is_contiguous()
                                      or face_mask.device != ro.device):
            raise ValueError("intersect: face_mask must be a contiguous uint8 [F = %d] tensor on the tree's device" % self.faces.shape[0])
        R, dev = ro.shape[0], ro.device
        spec = {"tid": ((R,), I32), "t": ((R,), F32), "loc": ((R, 3), F32), "uv": ((R, 2), F32), "front": ((R,), torch.uint8)}
        out = {k: torch.empty(spec[k][0], dtype=spec[k][1], device=dev) for k in want}
        visited = torch.zeros(1, dtype=torch.int64, device=dev) if count else None
        if R > 0:
            self.ctx.check(self.ctx.lib.utx_bvh_intersect(self.ctx.handle, self.handle, ptr(ro), ptr(rd), R, ptr(out.get("tid")), ptr(out.get("t")), ptr(out.get("loc")),
                                                          ptr(out.get("uv")), ptr(out.get("front")), ptr(face_mask), ptr(visited), 1 if force_stack else 0,
                                                          self.ctx.stream()))
        return (out, int(visited.item())) if count else out

    def occluded(self, a, b, force_stack=False, count=False):
        """utx_bvh_occluded: blocked [R] u8 for the segments a -> b ([R,3] each): 1 iff some triangle is hit with 0 <= t < 1 along b - a"""
        a, b = self._rows("occluded: a", a), self._rows("occluded: b", b)
        if a.shape != b.shape:
            raise ValueError("occluded: a is %s, b %s" % (tuple(a.shape), tuple(b.shape)))
        R = a.shape[0]
        blocked = torch.empty(R, dtype=torch.uint8, device=a.device)
        visited = torch.zeros(1, dtype=torch.int64, device=a.device) if count else None
        if R > 0:
            self.ctx.check(self.ctx.lib.utx_bvh_occluded(self.ctx.handle, self.handle, ptr(a), ptr(b), R, ptr(blocked), ptr(visited), 1 if force_stack else 0,
                                                         self.ctx.stream()))
        return (blocked, int(visited.item())) if count else blocked

    def points_enclosed(self, points, n_rays, seed, dirs=None, early_exit=True, stream_id=0, want_hits=False, force_stack=False):
        """utx_points_enclosed: inner [N] u8 = 1 iff each of the point's n_rays (1 .. 1024) rays hits the mesh (t >= 0, any hit).  The directions are the stream
        of sphere_directions(N, n_rays, seed, stream_id) -- or dirs [N,n_rays,3], read in its place.  early_exit: a point's remaining rays are dropped at its
        first miss (same inner).  want_hits: also hits [N] i32, the number of rays that hit -- exact only with early_exit=False."""
        points = self._rows("points_enclosed: points", points)
        n_rays = int(n_rays)
        if not 1 <= n_rays <= 1024:
            raise ValueError("points_enclosed: n_rays is %d, expected 1 .. 1024" % n_rays)
        N = points.shape[0]
        if dirs is not None:
            dirs = self._rows("points_enclosed: dirs", dirs, (n_rays, 3))
            if dirs.shape[0] != N:
                raise ValueError("points_enclosed: dirs is %s for %d points" % (tuple(dirs.shape), N))
        inner = torch.empty(N, dtype=torch.uint8, device=points.device)
        hits = torch.empty(N, dtype=I32, device=points.device) if want_hits else None
        if N > 0:
            self.ctx.check(self.ctx.lib.utx_points_enclosed(self.ctx.handle, self.handle, ptr(points), N, n_rays, int(seed) & (2 ** 64 - 1), int(stream_id) & 0xffffffff,
                                                            ptr(dirs), ptr(inner), ptr(hits), None, (1 if force_stack else 0) | (0 if early_exit else 2),
                                                            self.ctx.stream()))
        return (inner, hits) if want_hits else inner

    def sphere_directions(self, n_points, n_rays, seed, stream_id=0):
        """utx_sphere_directions: [n_points, n_rays, 3] f32, the unit directions points_enclosed draws for (point, ray) under (seed, stream_id)"""
        return sphere_directions(n_points, n_rays, seed, stream_id, device=self.verts.device)


def sphere_directions(n_points, n_rays, seed, stream_id=0, device=None):
    """utx_sphere_directions: [n_points, n_rays, 3] f32 -- Philox4x32-10 keyed by seed, counter (point, ray, attempt, stream_id), Marsaglia's rejection method"""
    n_points, n_rays = int(n_points), int(n_rays)
    if n_points < 0 or n_rays < 0 or not n_points * n_rays < 2 ** 31:
        raise ValueError("sphere_directions: %d x %d directions, expected counts >= 0 with a product < 2^31" % (n_points, n_rays))
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    ctx = get_ctx(dev.index)
    out = torch.empty(n_points, n_rays, 3, dtype=F32, device=dev)
    if out.numel() > 0:
        ctx.check(ctx.lib.utx_sphere_directions(ctx.handle, n_points, n_rays, int(seed) & (2 ** 64 - 1), int(stream_id) & 0xffffffff, ptr(out), ctx.stream()))
    return out


def backproject(rast2d, verts, faces, fnormal, vndc, dirs, images, bvh, angle_deg=100.0, view_begin=0, view_count=None,
                out=None, eyes=None, sample="grid"):
    """fused per-(view, texel) gather + visibility.  Returns color [n,Th,Tw,3], rayvis [n,Th,Tw] u8, alphaok u8.
    eyes None: orthographic rays along dirs [n,3] (utx_backproject); eyes [n,3] = c2w[:, :3, 3]: perspective rays from the camera
    centres (utx_backproject_persp; dirs is not read and may be None).
    sample: 'grid' -- grid_sample, bilinear, zero padding (grid_interpolate_mode='torch'); 'nvdiff' -- nvdiffrast's linear filtering with
    the wrap boundary (grid_interpolate_mode='nvdiff', utx_backproject_sampled(sample_mode=1))."""
    assert sample in ("grid", "nvdiff"), "sample must be 'grid' or 'nvdiff', not %r" % (sample,)
    ctx = get_ctx(rast2d.device.index)
    Th, Tw = rast2d.shape[:2]
    n, H, W = images.shape[:3]
    dev = rast2d.device
    if out is None:
        color = torch.zeros(n, Th, Tw, 3, dtype=F32, device=dev)
        rayvis = torch.zeros(n, Th, Tw, dtype=U8, device=dev)
        alphaok = torch.zeros(n, Th, Tw, dtype=U8, device=dev)
    else:
        color, rayvis, alphaok = out
    d = BackprojectDesc()
    d.rast2d, d.verts, d.faces, d.fnormal = ptr(_f(rast2d)), ptr(_f(verts)), ptr(_i(faces)), ptr(_f(fnormal))
    d.vndc, d.images = ptr(_f(vndc)), ptr(_f(images))
    if eyes is None:
        d.dirs = ptr(_f(dirs))
    d.color, d.rayvis, d.alphaok = ptr(color), ptr(rayvis), ptr(alphaok)
    d.T_h, d.T_w, d.V, d.n_views, d.H, d.W = Th, Tw, verts.shape[0], n, H, W
    d.view_begin, d.view_count = view_begin, (n - view_begin if view_count is None else view_count)
    d.cos_thresh = float(np.float32(math.cos(math.radians(angle_deg))))
    d.two_sqrt3 = float(np.float32(2.0 * math.sqrt(3.0)))
    if eyes is not None:
        assert eyes.shape == (n, 3)
    if sample == "nvdiff":
        ctx.check(ctx.lib.utx_backproject_sampled(ctx.handle, C.byref(d), None if eyes is None else ptr(_f(eyes)), 1, bvh.handle, ctx.stream()))
    elif eyes is None:
        ctx.check(ctx.lib.utx_backproject(ctx.handle, C.byref(d), bvh.handle, ctx.stream()))
    else:
        ctx.check(ctx.lib.utx_backproject_persp(ctx.handle, C.byref(d), ptr(_f(eyes)), bvh.handle, ctx.stream()))
    return color, rayvis, alphaok


def dilate_visibility(rayvis, alphaok, rast2d):
    ctx = get_ctx(rayvis.device.index)
    n, H, W = rayvis.shape
    tmp = torch.empty_like(rayvis)
    out = torch.empty_like(rayvis)
    ctx.check(ctx.lib.utx_dilate_visibility(ctx.handle, ptr(rayvis), ptr(alphaok), ptr(_f(rast2d)), n, H, W, ptr(tmp), ptr(out), ctx.stream()))
    return out


def composite(colors, vis, order):
    ctx = get_ctx(colors.device.index)
    n, H, W = vis.shape
    atlas = torch.empty(H, W, 3, dtype=F32, device=colors.device)
    winner = torch.empty(H, W, dtype=torch.int8, device=colors.device)
    arr = (C.c_int * len(order))(*order)
    ctx.check(ctx.lib.utx_composite(ctx.handle, ptr(_f(colors)), ptr(vis), arr, len(order), H * W, ptr(atlas), ptr(winner), ctx.stream()))
    return atlas, winner


SEAM_RADIUS_MAX = 15      # k_boundary // 2 and k_boundary_blur // 2 (utx_seam_mask_sized)
GAUSS_KSIZE_MAX = 31      # utx_gaussian_blur_seam


def seam_mask(winner, rast2d, k_boundary=3, k_boundary_blur=3):
    """winner [H,W] int8 (composite), rast2d [H,W,4] -> seam [H,W] u8 (bake_mv_to_uv_reproject_blur's boundary mask, :596-604):
    the winner boundary within radius k_boundary // 2, dilated by k_boundary_blur // 2, inside the coverage eroded by k_boundary_blur // 2 + 2.
    The defaults (3, 3) run utx_seam_mask; other sizes utx_seam_mask_sized (both radii <= 15)."""
    ctx = get_ctx(winner.device.index)
    H, W = winner.shape
    seam = torch.empty(H, W, dtype=U8, device=winner.device)
    if k_boundary == 3 and k_boundary_blur == 3:
        tmp = torch.empty(H, W, dtype=U8, device=winner.device)
        ctx.check(ctx.lib.utx_seam_mask(ctx.handle, ptr(winner), ptr(_f(rast2d)), H, W, ptr(tmp), ptr(seam), ctx.stream()))
    else:
        tmp = torch.empty(4, H, W, dtype=U8, device=winner.device)
        ctx.check(ctx.lib.utx_seam_mask_sized(ctx.handle, ptr(winner), ptr(_f(rast2d)), H, W, int(k_boundary), int(k_boundary_blur), ptr(tmp),
                                              ptr(seam), ctx.stream()))
    return seam


def view_visibility(attr6, rast, fnormal, dirs, grad_thr=0.20, angle_deg=115.0, radius=15, eyes=None):
    """mv_to_pcd's filt_gradient_points=True visibility (renderer_inverse.py:189-209): attr6 [n,H,W,6] interpolated
    (position, vertex normal), rast [n,H,W,4], dirs [n,3] ray directions -> (vis u8 [n,H,W], alpha f32 [n,H,W]).
    eyes [n,3] = c2w[:, :3, 3] (dirs then unused, may be None): perspective, each pixel's ray runs from the camera centre to its position."""
    ctx = get_ctx(rast.device.index)
    n, H, W, _ = rast.shape
    tmp = torch.empty(2 * n * H * W, dtype=U8, device=rast.device)
    vis = torch.empty(n, H, W, dtype=U8, device=rast.device)
    alpha = torch.empty(n, H, W, dtype=F32, device=rast.device)
    cos_thr = float(np.float32(math.cos(math.radians(angle_deg))))
    if eyes is None:
        ctx.check(ctx.lib.utx_view_visibility(ctx.handle, ptr(_f(attr6)), ptr(_f(rast)), ptr(_f(fnormal)), ptr(_f(dirs)), n, H, W,
                                              float(grad_thr), cos_thr, int(radius), ptr(tmp), ptr(vis), ptr(alpha), ctx.stream()))
    else:
        assert eyes.shape == (n, 3)
        ctx.check(ctx.lib.utx_view_visibility_persp(ctx.handle, ptr(_f(attr6)), ptr(_f(rast)), ptr(_f(fnormal)), ptr(_f(eyes)), n, H, W,
                                                    float(grad_thr), cos_thr, int(radius), ptr(tmp), ptr(vis), ptr(alpha), ctx.stream()))
    return vis, alpha


def knn_gather(src_pos, dst_pos, k, src_attr=None, src_mask=None, dst_mask=None, out=None, mode="mean", src_nrm=None, dst_nrm=None,
               want_index=False, out_index=None):
    """exact k-NN in 3-D over dense, byte-masked point sets (bake_mv_to_uv_kdtree, renderer_inverse.py:367-433).
    src_pos [N,3], dst_pos [M,3]; src_attr [N,C] -> out [M,C] (written only where dst_mask): mean of the k neighbours'
    attributes, or the MVPaint weighting (mode='mvpaint').  want_index: also return (idx [M,k] i32, d2 [M,k] f32).
    out_index: a pair of contiguous tensors (idx, d2) of those shapes and types on src_pos's device, written in place and returned as with
    want_index (rows outside dst_mask keep their contents)."""
    from .._lib import KnnDesc
    ctx = get_ctx(src_pos.device.index)
    dev = src_pos.device
    src_pos, dst_pos = _f(src_pos).reshape(-1, 3), _f(dst_pos).reshape(-1, 3)
    N, M = src_pos.shape[0], dst_pos.shape[0]
    d = KnnDesc()
    keep = [src_pos, dst_pos]
    d.src_pos, d.dst_pos, d.N, d.M, d.k = ptr(src_pos), ptr(dst_pos), N, M, int(k)
    d.mode = {"mean": 0, "mvpaint": 1}[mode]
    if src_attr is not None:
        src_attr = _f(src_attr).reshape(N, -1)
        d.C = src_attr.shape[1]
        if out is None:
            out = torch.zeros(M, d.C, dtype=F32, device=dev)
        assert out.is_contiguous() and out.dtype == F32 and out.numel() == M * d.C
        d.src_attr, d.out_attr = ptr(src_attr), ptr(out)
        keep += [src_attr, out]
    for name, t in (("src_mask", src_mask), ("dst_mask", dst_mask)):
        if t is not None:
            t = t.reshape(-1).to(U8).contiguous()
            keep.append(t)
            setattr(d, name, ptr(t))
    for name, t in (("src_nrm", src_nrm), ("dst_nrm", dst_nrm)):
        if t is not None:
            t = _f(t).reshape(-1, 3)
            keep.append(t)
            setattr(d, name, ptr(t))
    idx = d2 = None
    if out_index is not None:
        idx, d2 = out_index
        for name, t, dt in (("idx", idx, I32), ("d2", d2, F32)):
            if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.device == dev and t.is_contiguous() and t.numel() == M * int(k)):
                raise ValueError("out_index: %s must be a contiguous %s tensor of %d x %d elements on %s" % (name, dt, M, int(k), dev))
        d.out_idx, d.out_d2 = ptr(idx), ptr(d2)
    elif want_index:
        idx = torch.empty(M, int(k), dtype=I32, device=dev)
        d2 = torch.empty(M, int(k), dtype=F32, device=dev)
        d.out_idx, d.out_d2 = ptr(idx), ptr(d2)
    wb = ctx.lib.utx_knn_workspace_bytes(N)
    work = torch.empty(wb, dtype=U8, device=dev)
    ctx.check(ctx.lib.utx_knn(ctx.handle, C.byref(d), ptr(work), wb, ctx.stream()))
    if want_index or out_index is not None:
        return out, idx, d2
    return out


def fps(pos, n_samples, mask=None, start=0, want_d2=False):
    """exact farthest-point sampling (utx_fps): pos [N,3] f32, mask [N] (optional) -> idx [n_samples] i32 (-1 behind the last candidate); want_d2: also each
    pick's squared distance to the set chosen before it (+inf for the first, -1 behind the last candidate).  start: first pick, -1 = lowest valid index."""
    ctx = get_ctx(pos.device.index)
    pos = _f(pos).reshape(-1, 3)
    if pos.data_ptr() % 16:
        pos = pos.clone()
    N, M, start = pos.shape[0], int(n_samples), int(start)
    if M <= 0:
        raise ValueError("farthest-point sampling needs n_samples > 0, got %d" % M)
    if not 0 < N < 2 ** 31:
        raise ValueError("farthest-point sampling takes 0 < N < 2^31 points, got %d" % N)
    if not -1 <= start < N:
        raise ValueError("start index %d is outside [-1, %d)" % (start, N))
    if mask is not None:
        mask = mask.reshape(-1).to(U8).contiguous()
        assert mask.numel() == N
    idx = torch.empty(M, dtype=I32, device=pos.device)
    d2 = torch.empty(M, dtype=F32, device=pos.device) if want_d2 else None
    wb = ctx.lib.utx_fps_workspace_bytes(N)
    work = torch.empty(wb, dtype=U8, device=pos.device)
    ctx.check(ctx.lib.utx_fps(ctx.handle, ptr(pos), ptr(mask), N, M, start, ptr(idx), ptr(d2), ptr(work), wb, ctx.stream()))
    return (idx, d2) if want_d2 else idx


def sample_edges_equal_steps(verts, edges, start, length, total, N, edge_ids=None):
    """sample_on_edges_v2's sampling (utx_sample_edges_equal_steps): verts [V,3] f32, edges [E,2] i32 (selected), start / length [E] f32, total float
    -> samples [N,3] f32, edge_index [N] i32 (edge_ids[e] when given, else e), edge_t [N] f32."""
    ctx = get_ctx(verts.device.index)
    E, N = edges.shape[0], int(N)
    assert start.shape == (E,) and length.shape == (E,) and (edge_ids is None or edge_ids.shape == (E,))
    samples = torch.empty(N, 3, dtype=F32, device=verts.device)
    eidx = torch.empty(N, dtype=I32, device=verts.device)
    et = torch.empty(N, dtype=F32, device=verts.device)
    ctx.check(ctx.lib.utx_sample_edges_equal_steps(ctx.handle, ptr(_f(verts)), ptr(_i(edges)), ptr(_i(edge_ids) if edge_ids is not None else None), ptr(_f(start)),
                                                   ptr(_f(length)), E, float(total), N, ptr(samples), ptr(eidx), ptr(et), ctx.stream()))
    return samples, eidx, et


def sample_surface(verts, faces, cum, N, seed):
    """sample_surface's sampling on the defined Philox4x32-10 stream (utx_sample_surface): verts [V,3] f32, faces [F,3] i32, cum [F] f32 running face weights
    -> samples [N,3] f32, face_index [N] i32, uvw [N,3] f32."""
    ctx = get_ctx(verts.device.index)
    F, N = faces.shape[0], int(N)
    assert cum.shape == (F,)
    samples = torch.empty(N, 3, dtype=F32, device=verts.device)
    fidx = torch.empty(N, dtype=I32, device=verts.device)
    uvw = torch.empty(N, 3, dtype=F32, device=verts.device)
    ctx.check(ctx.lib.utx_sample_surface(ctx.handle, ptr(_f(verts)), ptr(_i(faces)), ptr(_f(cum)), F, N, int(seed) & (2 ** 64 - 1), ptr(samples), ptr(fidx), ptr(uvw),
                                         ctx.stream()))
    return samples, fidx, uvw


CLOSEST_POINT_OUTPUTS = ("dist", "face", "uvw", "closest")


def closest_point(bvh, points, want=CLOSEST_POINT_OUTPUTS, brute=False, count=False, seed_descent=True):
    """utx_bvh_closest_point: the nearest point of the mesh of `bvh` (ops.BVH) to every row of points [N,3] f32 -> dict of the buffers named in `want`:
    dist [N] f32 (the distance, not its square), face [N] i32 (-1 for a query with a non-finite coordinate), uvw [N,3] f32 weighing the face's corners,
    closest [N,3] f32.  The face with the smallest squared distance, ties to the smallest id.  brute: the exhaustive loop over all faces instead of the tree walk
    (equal results); seed_descent=False: the walk without its greedy first descent (equal results); count: also return the number of tree nodes visited."""
    points = _f(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("closest_point: points is %s, expected [N, 3]" % (tuple(points.shape),))
    want = tuple(want)
    for k in want:
        if k not in CLOSEST_POINT_OUTPUTS:
            raise ValueError("closest_point: unknown output %r (one of %s)" % (k, ", ".join(CLOSEST_POINT_OUTPUTS)))
    ctx, N, dev = bvh.ctx, points.shape[0], points.device
    if not N < 2 ** 31:
        raise ValueError("closest_point takes N < 2^31 points, got %d" % N)
    out = {"dist": torch.empty(N, dtype=F32, device=dev)}
    if "face" in want:
        out["face"] = torch.empty(N, dtype=I32, device=dev)
    for k in ("uvw", "closest"):
        if k in want:
            out[k] = torch.empty(N, 3, dtype=F32, device=dev)
    visited = torch.zeros(1, dtype=torch.int64, device=dev) if count else None
    if N > 0:
        ctx.check(ctx.lib.utx_bvh_closest_point(ctx.handle, bvh.handle, ptr(points), N, ptr(out["dist"]), ptr(out.get("face")), ptr(out.get("uvw")),
                                                ptr(out.get("closest")), ptr(visited) if count else None, (1 if brute else 0) | (0 if seed_descent else 2),
                                                ctx.stream()))
    out = {k: out[k] for k in want}
    return (out, int(visited.item())) if count else out


def sample_offsets(N, seed, stream_id, base=None, faces=None, face_index=None, uvw=None, vnormal=None, threshold=0.0, uniforms=None):
    """utx_sample_offsets: N points of the random stream `stream_id` (Philox4x32-10, counter (i, stream_id, 0, 0)).  base None: the points themselves, in [0, 1)^3.
    Otherwise base [N,3] + (threshold * (2 r - 1)) * n with n the vertex normals vnormal [V,3] interpolated by (face_index [N] i32, uvw [N,3]) over faces [F,3] i32.
    uniforms [N,3] (tests): read in place of the stream."""
    N = int(N)
    some = base if base is not None else uniforms
    dev = some.device if some is not None else torch.device("cuda", torch.cuda.current_device())
    ctx = get_ctx(dev.index)
    out = torch.empty(N, 3, dtype=F32, device=dev)
    if base is not None:
        assert tuple(base.shape) == (N, 3) and tuple(uvw.shape) == (N, 3) and tuple(face_index.shape) == (N,) and faces.dim() == 2 and vnormal.dim() == 2
    if uniforms is not None:
        assert tuple(uniforms.shape) == (N, 3)
    ctx.check(ctx.lib.utx_sample_offsets(ctx.handle, ptr(_f(base)) if base is not None else None, ptr(_i(faces)) if base is not None else None,
                                         faces.shape[0] if base is not None else 0, ptr(_i(face_index)) if base is not None else None,
                                         ptr(_f(uvw)) if base is not None else None, ptr(_f(vnormal)) if base is not None else None,
                                         ptr(_f(uniforms)) if uniforms is not None else None, N, int(seed) & (2 ** 64 - 1), int(stream_id), float(threshold),
                                         ptr(out) if N else None, ctx.stream()))
    return out


SAMPLE_ATTRS_MAX = 4


def sample_attrs(attrs, face_index, uvw, faces=None, faces_2d=None, uvs_2d=None):
    """utx_sample_attrs: PBRMesh.__call__ of the reference for up to four attributes in one launch.  attrs: dict name -> f32 tensor, a constant [C], a per-vertex
    array [V,C] (needs faces [F,3] i32) or a texture [H,W,C] with C <= 4 (needs faces_2d [F,3] i32 and uvs_2d [V2,2] f32; the interpolated uv is grid_sample's
    grid coordinate as it stands, bilinear, align_corners=False, reflection padding).  face_index [N] i32, uvw [N,3] f32 -> dict name -> [N,C] f32."""
    if (faces_2d is None) != (uvs_2d is None):
        raise ValueError("sample_attrs: faces_2d and uvs_2d go together, got only %s" % ("faces_2d" if uvs_2d is None else "uvs_2d"))
    names = list(attrs)
    if not 1 <= len(names) <= SAMPLE_ATTRS_MAX:
        raise ValueError("sample_attrs takes 1 to %d attributes, got %d" % (SAMPLE_ATTRS_MAX, len(names)))
    face_index, uvw = _i(face_index), _f(uvw)
    N, dev = face_index.shape[0], face_index.device
    if tuple(uvw.shape) != (N, 3):
        raise ValueError("sample_attrs: uvw is %s, expected [%d, 3]" % (tuple(uvw.shape), N))
    ctx = get_ctx(dev.index)
    F = None
    for t in (faces, faces_2d):
        if t is not None:
            if t.dim() != 2 or t.shape[1] != 3 or (F is not None and t.shape[0] != F):
                raise ValueError("sample_attrs: faces / faces_2d must be [F, 3] with one F")
            F = t.shape[0]
    src, dims, out = [], [], {}
    for k in names:
        a = _f(attrs[k])
        if a.dim() == 1:
            kind, Cc, H, W = 0, a.shape[0], 0, 0
        elif a.dim() == 2:
            kind, Cc, H, W = 1, a.shape[1], 0, 0
            if faces is None:
                raise ValueError("sample_attrs: %s is per-vertex and needs faces" % k)
        elif a.dim() == 3:
            kind, Cc, H, W = 2, a.shape[2], a.shape[0], a.shape[1]
            if faces_2d is None or uvs_2d is None:
                raise ValueError("sample_attrs: %s is a texture and needs faces_2d and uvs_2d" % k)
            if Cc > 4 or H < 1 or W < 1:
                raise ValueError("sample_attrs: texture %s is %s, expected [H >= 1, W >= 1, C <= 4]" % (k, tuple(a.shape)))
        else:
            raise NotImplementedError("invalid shape of %s: %s" % (k, tuple(a.shape)))
        if not 1 <= Cc <= 16:
            raise ValueError("sample_attrs: %s has %d channels, expected 1 to 16" % (k, Cc))
        src.append(a)
        dims += [kind, Cc, H, W]
        out[k] = torch.empty(N, Cc, dtype=F32, device=dev)
    if N == 0:
        return out
    n = len(names)
    sp = (C.c_void_p * n)(*[a.data_ptr() for a in src])
    op = (C.c_void_p * n)(*[out[k].data_ptr() for k in names])
    dm = (C.c_int * (4 * n))(*[int(d) for d in dims])
    ctx.check(ctx.lib.utx_sample_attrs(ctx.handle, ptr(_i(faces)) if faces is not None else None, ptr(_i(faces_2d)) if faces_2d is not None else None,
                                       ptr(_f(uvs_2d)) if uvs_2d is not None else None, F if F is not None else 1, ptr(face_index), ptr(uvw), N, n, sp, dm, op,
                                       ctx.stream()))
    return out


# ---- atlas post-processing.  Every image is interleaved [H,W,C] f32, 1 <= C <= CHANNELS_MAX, each channel on its own: a channel's result does not depend on
# C or on where in the image it sits.  C == 3 goes through the 3-channel entries of the C ABI, any other C through the *_c entries (one library routine behind both).
CHANNELS_MAX = 16


def nn_fill(atlas, winner, rast2d, pos, want_index=False):
    """in place on atlas [H,W,C]; want_index: returns the search's nn_index [H*W] i32 (-1 where the texel was not filled)"""
    ctx = get_ctx(atlas.device.index)
    H, W = winner.shape
    T = H * W
    Cc = atlas.shape[-1]
    wb = ctx.lib.utx_nn_fill_workspace_bytes(T)
    work = torch.empty(wb, dtype=U8, device=atlas.device)
    idx = torch.empty(T, dtype=I32, device=atlas.device) if (want_index or Cc != 3) else None      # utx_nn_fill_c copies from the index
    if Cc == 3:
        ctx.check(ctx.lib.utx_nn_fill(ctx.handle, ptr(_f(pos)), ptr(winner), ptr(_f(rast2d)), T, ptr(_f(atlas)), ptr(idx), ptr(work), wb, ctx.stream()))
    else:
        ctx.check(ctx.lib.utx_nn_fill_c(ctx.handle, ptr(_f(pos)), ptr(winner), ptr(_f(rast2d)), T, Cc, ptr(_f(atlas)), ptr(idx), ptr(work), wb, ctx.stream()))
    return idx if want_index else None


def lens_blur_kernel49(radius=3.0):
    """Collapse the 5 separable complex components of lens_blur_torch (image/lens_blur.py:62-112,190-212)
    into one real 7x7 kernel: K = sum_c A_c Re(k_c (x) k_c) + B_c Im(k_c (x) k_c)  (host, float32)."""
    params = [[4.892608, 1.685979, -22.356787, 85.91246], [4.71187, 4.998496, 35.918936, -28.875618],
              [4.052795, 8.244168, -13.212253, -1.578428], [2.929212, 11.900859, 0.507991, 1.816328],
              [1.512961, 16.116382, 0.138051, -0.01]]
    scale = 1.2
    kr = int(math.ceil(radius))
    n = 2 * kr + 1
    ax = np.linspace(-radius, radius, n, dtype=np.float32) * np.float32(scale) * np.float32(1 / radius)
    ks = []
    for a, b, A, B in params:
        re = (np.exp(-a * ax ** 2) * np.cos(b * ax ** 2)).astype(np.float32)
        im = (np.exp(-a * ax ** 2) * np.sin(b * ax ** 2)).astype(np.float32)
        ks.append((re, im, A, B))
    total = 0.0
    for re, im, A, B in ks:
        total += float(np.sum(A * (np.outer(re, re) - np.outer(im, im)) + B * (np.outer(re, im) + np.outer(im, re))))
    K = np.zeros((n, n), dtype=np.float64)
    for re, im, A, B in ks:
        re64, im64 = re.astype(np.float64), im.astype(np.float64)
        K += A * (np.outer(re64, re64) - np.outer(im64, im64)) + B * (np.outer(re64, im64) + np.outer(im64, re64))
    return (K / total).astype(np.float32)


def lens_blur_seam(src, seam, k49=None):
    """src [H,W,C] f32, seam [H,W] u8 -> dst: the collapsed lens blur where seam is set, src elsewhere"""
    ctx = get_ctx(src.device.index)
    H, W = seam.shape
    if k49 is None:
        k49 = lens_blur_kernel49()
    arr = (C.c_float * 49)(*[float(x) for x in np.asarray(k49, dtype=np.float32).reshape(-1)])
    dst = torch.empty_like(src)
    Cc = src.shape[-1]
    if Cc == 3:
        ctx.check(ctx.lib.utx_lens_blur_seam(ctx.handle, ptr(_f(src)), ptr(seam), H, W, arr, ptr(dst), ctx.stream()))
    else:
        ctx.check(ctx.lib.utx_lens_blur_seam_c(ctx.handle, ptr(_f(src)), ptr(seam), H, W, Cc, arr, ptr(dst), ctx.stream()))
    return dst


def gaussian_kernel1d(ksize):
    """the 1-D weights of torchvision's gaussian_blur(img, (k, k)) with sigma=None, built the way it builds them (torch, float32, CPU):
    sigma = 0.15 k + 0.35, x = linspace(-(k-1)/2, (k-1)/2, k), pdf = exp(-0.5 (x / sigma)^2), w = pdf / pdf.sum()."""
    sigma = ksize * 0.15 + 0.35
    half = (ksize - 1) * 0.5
    x = torch.linspace(-half, half, steps=ksize, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_blur_seam(src, seam, ksize=5):
    """src [H,W,C] f32, seam [H,W] u8 -> dst: torchvision's gaussian_blur(src, (ksize, ksize)) (reflect padding) where seam is set, src
    elsewhere (bake_mv_to_uv_reproject_blur(method='gaussian'), :618-625).  ksize odd, 1..31, ksize // 2 < min(H, W)."""
    ctx = get_ctx(src.device.index)
    H, W = seam.shape
    w1 = gaussian_kernel1d(int(ksize))
    arr = (C.c_float * int(ksize))(*[float(x) for x in w1.numpy()])
    dst = torch.empty_like(src)
    Cc = src.shape[-1]
    if Cc == 3:
        ctx.check(ctx.lib.utx_gaussian_blur_seam(ctx.handle, ptr(_f(src)), ptr(seam), H, W, int(ksize), arr, ptr(dst), ctx.stream()))
    else:
        ctx.check(ctx.lib.utx_gaussian_blur_seam_c(ctx.handle, ptr(_f(src)), ptr(seam), H, W, Cc, int(ksize), arr, ptr(dst), ctx.stream()))
    return dst


def pull_push(kd, mask):
    """kd [H,W,C] f32, mask [H,W] u8 -> [H,W,C]"""
    ctx = get_ctx(kd.device.index)
    H, W = mask.shape
    Cc = kd.shape[-1]
    wb = ctx.lib.utx_pull_push_workspace_bytes(H, W) if Cc == 3 else ctx.lib.utx_pull_push_workspace_bytes_c(H, W, Cc)
    work = torch.empty(max(wb, 1), dtype=U8, device=kd.device)
    out = torch.empty_like(kd)
    if Cc == 3:
        ctx.check(ctx.lib.utx_pull_push(ctx.handle, ptr(_f(kd)), ptr(mask), H, W, ptr(out), ptr(work), ctx.stream()))
    else:
        ctx.check(ctx.lib.utx_pull_push_c(ctx.handle, ptr(_f(kd)), ptr(mask), H, W, Cc, ptr(out), ptr(work), ctx.stream()))
    return out


# ---- the C-channel (PBR stack) bake: visibility and winner without colour, one gather from the winning view (images interleaved [..., C] f32, 1 <= C <= CHANNELS_MAX)


def backproject_vis(rast2d, verts, faces, fnormal, vndc, dirs, alpha, bvh, angle_deg=100.0, view_begin=0, view_count=None, out=None, eyes=None,
                    sample="grid"):
    """backproject() without the colour gather (utx_backproject_vis): alpha [n,H,W] f32 is the plane the texels sample.
    Returns rayvis, alphaok [n,Th,Tw] u8 -- bit-identical to backproject()'s on images whose fourth channel is alpha."""
    assert sample in ("grid", "nvdiff"), "sample must be 'grid' or 'nvdiff', not %r" % (sample,)
    ctx = get_ctx(rast2d.device.index)
    Th, Tw = rast2d.shape[:2]
    n, H, W = alpha.shape
    dev = rast2d.device
    if out is None:
        rayvis = torch.zeros(n, Th, Tw, dtype=U8, device=dev)
        alphaok = torch.zeros(n, Th, Tw, dtype=U8, device=dev)
    else:
        rayvis, alphaok = out
    d = BackprojectDesc()
    d.rast2d, d.verts, d.faces, d.fnormal = ptr(_f(rast2d)), ptr(_f(verts)), ptr(_i(faces)), ptr(_f(fnormal))
    d.vndc, d.images = ptr(_f(vndc)), ptr(_f(alpha))
    if eyes is None:
        d.dirs = ptr(_f(dirs))
    else:
        assert eyes.shape == (n, 3)
    d.rayvis, d.alphaok = ptr(rayvis), ptr(alphaok)
    d.T_h, d.T_w, d.V, d.n_views, d.H, d.W = Th, Tw, verts.shape[0], n, H, W
    d.view_begin, d.view_count = view_begin, (n - view_begin if view_count is None else view_count)
    d.cos_thresh = float(np.float32(math.cos(math.radians(angle_deg))))
    d.two_sqrt3 = float(np.float32(2.0 * math.sqrt(3.0)))
    ctx.check(ctx.lib.utx_backproject_vis(ctx.handle, C.byref(d), None if eyes is None else ptr(_f(eyes)), 1 if sample == "nvdiff" else 0, bvh.handle,
                                          ctx.stream()))
    return rayvis, alphaok


def composite_winner(vis, order):
    """vis [n,H,W] u8 -> winner [H,W] int8: the first view of `order` that sees the texel, -1 where none does (composite() without colours)"""
    ctx = get_ctx(vis.device.index)
    n, H, W = vis.shape
    assert vis.dtype == U8 and vis.is_contiguous()
    winner = torch.empty(H, W, dtype=torch.int8, device=vis.device)
    arr = (C.c_int * len(order))(*order)
    ctx.check(ctx.lib.utx_composite_winner(ctx.handle, ptr(vis), n, arr, len(order), H * W, ptr(winner), ctx.stream()))
    return winner


def gather_winner(rast2d, faces, vndc, images, winner, sample="grid"):
    """atlas [Th,Tw,C]: images [n,H,W,C] sampled at every texel's NDC in its winning view (zeros where winner < 0), as backproject() samples"""
    assert sample in ("grid", "nvdiff"), "sample must be 'grid' or 'nvdiff', not %r" % (sample,)
    ctx = get_ctx(rast2d.device.index)
    Th, Tw = rast2d.shape[:2]
    n, H, W, Cc = images.shape
    assert vndc.shape[0] == n and winner.shape == (Th, Tw) and winner.dtype == torch.int8 and winner.is_contiguous()
    atlas = torch.empty(Th, Tw, Cc, dtype=F32, device=rast2d.device)
    ctx.check(ctx.lib.utx_gather_winner(ctx.handle, ptr(_f(rast2d)), ptr(_i(faces)), ptr(_f(vndc)), ptr(_f(images)), ptr(winner), Th * Tw, vndc.shape[1], n,
                                        H, W, Cc, 1 if sample == "nvdiff" else 0, ptr(atlas), ctx.stream()))
    return atlas


def to_u8(img, flip=False):
    ctx = get_ctx(img.device.index)
    rows = img.shape[0]
    row_elems = img.numel() // rows
    out = torch.empty(img.shape, dtype=U8, device=img.device)
    ctx.check(ctx.lib.utx_to_u8(ctx.handle, ptr(_f(img)), rows, row_elems, int(flip), ptr(out), ctx.stream()))
    return out


# ---- the vertex-colour bake (vertex_bake.hip): project_vertex_color / remapping_vertex_color / inpainting_vertex_color of the reference

VERTEX_BLENDING = {None: 0, "soft": 1, "hard": 2}      # UTX_VB_BLEND_*


def weight_map_radius(render_size):
    """the dilation radius of the edge alpha: the reference's kernel_size = 2 * (render_size // 512) + 1 is (2 r + 1) with r = render_size // 512"""
    return int(render_size) // 512


def view_weight_maps(cos_ray_normal, camera_normal=None, r=0, want_arccos=False):
    """utx_view_weight_maps: cos_ray_normal [B,H,W,1] (or [B,H,W]) -> [B,H,W,2] = (cos term, edge alpha dilated by r), the two weight channels of
    project_vertex_color (mesh_remapping.py:544-555).  camera_normal [B,H,W,3]: the orthographic cos term clamp(camera_normal.z, 0, 1) instead of
    clamp(cos, -1, 0).  want_arccos: also the arccos term in [0, 1] the edge alpha is the gradient of, [B,H,W]."""
    ctx = get_ctx(cos_ray_normal.device.index)
    B, H, W = cos_ray_normal.shape[:3]
    assert cos_ray_normal.numel() == B * H * W, "cos_ray_normal is [B, H, W, 1]"
    assert camera_normal is None or tuple(camera_normal.shape) == (B, H, W, 3), "camera_normal is [B, H, W, 3]"
    out = torch.empty(B, H, W, 2, dtype=F32, device=cos_ray_normal.device)
    tmp = torch.empty(B * H * W, dtype=U8, device=out.device) if r > 0 else None
    arccos = torch.empty(B, H, W, dtype=F32, device=out.device) if want_arccos else None
    ctx.check(ctx.lib.utx_view_weight_maps(ctx.handle, ptr(_f(cos_ray_normal)), _opt(camera_normal), B, H, W, int(r), ptr(tmp), ptr(out), ptr(arccos), ctx.stream()))
    return (out, arccos) if want_arccos else out


def _epilogue_args(epilogue, who):
    """the `epilogue` dict of vertex_project / uv_bake, checked -> its four C arguments (overlay_conf, blending, blending_conf, inpainting_conf); None: zeros"""
    e = dict(overlay_confidence=0.0, blending=None, blending_confidence=0.0, inpainting_confidence=0.0) if epilogue is None else epilogue
    if e["blending"] not in VERTEX_BLENDING:
        raise ValueError("%s: blending %r (None, 'soft' or 'hard')" % (who, e["blending"]))
    return float(e["overlay_confidence"]), VERTEX_BLENDING[e["blending"]], float(e["blending_confidence"]), float(e["inpainting_confidence"])


def vertex_project(v_pos, visible, xform, proj, images, wmap, v_rgb, weights, use_alpha=True, epilogue=None):
    """utx_vertex_project: v_pos [V,3], visible uint8 [B,V], xform / proj [B,4,4] (the per-view vertex transform and the projection), images
    [B,4,Hi,Wi] rgba, wmap [B,H,W,2] (view_weight_maps), v_rgb [V,3], weights [B] -> (v_rgb_acc [V,3], v_weight_acc [V,1]): the loop of
    project_vertex_color (:559-594), the views summed in index order.  epilogue = dict(overlay_confidence, blending (None | 'soft' | 'hard'),
    blending_confidence, inpainting_confidence): the same launch also applies remapping_vertex_color's overlay and blending (:326-337) and returns
    (v_rgb_acc, v_weight_acc, blended [V,3], inpaint_mask uint8 [V] = v_weight_acc <= inpainting_confidence)."""
    ctx = get_ctx(v_pos.device.index)
    V, B = v_pos.shape[0], visible.shape[0]
    assert tuple(visible.shape) == (B, V) and tuple(xform.shape) == (B, 4, 4) and tuple(proj.shape) == (B, 4, 4) and tuple(weights.shape) == (B,)
    assert images.dim() == 4 and images.shape[0] == B and images.shape[1] == 4, "images is [B, 4, Hi, Wi]"
    assert wmap.dim() == 4 and wmap.shape[0] == B and wmap.shape[3] == 2, "wmap is [B, H, W, 2]"
    assert tuple(v_rgb.shape) == (V, 3) and v_pos.shape[1] == 3
    dev = v_pos.device
    acc = torch.empty(V, 3, dtype=F32, device=dev)
    wacc = torch.empty(V, 1, dtype=F32, device=dev)
    head = (ctx.handle, ptr(_f(v_pos)), V, ptr(_u8(visible)), B, ptr(_f(xform)), ptr(_f(proj)), ptr(_f(images)), images.shape[2], images.shape[3], ptr(_f(wmap)),
            wmap.shape[1], wmap.shape[2], ptr(_f(v_rgb)), ptr(_f(weights)), int(bool(use_alpha)), ptr(acc), ptr(wacc))
    if epilogue is None:
        ctx.check(ctx.lib.utx_vertex_project(*head, ctx.stream()))
        return acc, wacc
    args = _epilogue_args(epilogue, "vertex_project")
    blended = torch.empty(V, 3, dtype=F32, device=dev)
    mask = torch.empty(V, dtype=U8, device=dev)
    ctx.check(ctx.lib.utx_vertex_project_blend(*head, *args, ptr(blended), ptr(mask), ctx.stream()))
    return acc, wacc, blended, mask


def vertex_adjacency(faces, V):
    """CSR vertex adjacency of a triangle mesh: faces [F,3] (any integer type, any device) -> (rowptr [V+1], col [nnz]) int32 on the faces' device; the
    unique undirected edges, both directions, every row's neighbours ascending (the pattern of Mesh.laplacian, mesh/structure.py:743-763)."""
    f = faces.long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e = torch.cat([e, e.flip(1)], 0)
    e = e[e[:, 0] != e[:, 1]]
    key = torch.unique(e[:, 0] * int(V) + e[:, 1])      # sorted: by row, then by neighbour
    row, col = key // int(V), key % int(V)
    rowptr = torch.zeros(int(V) + 1, dtype=torch.int64, device=faces.device)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=int(V)), 0)
    return rowptr.to(I32).contiguous(), col.to(I32).contiguous()


def vertex_inpaint(rowptr, col, v_rgb, v_idx, max_iters=1000, trace=None):
    """inpainting_vertex_color (:605-627) on the adjacency of vertex_adjacency: v_rgb [V,3], v_idx [n] the vertices to fill -> (v_rgb filled, number of
    steps).  One utx_vertex_inpaint_step launch per step, colour and mask double-buffered; after each step the host reads the 4-byte count of filled
    vertices back and stops when it did not grow (that last step is applied, as in the reference) or at max_iters.  No vertex to fill: no launch.
    v_idx must index the vertices (not checked here); a vertex listed twice is counted twice, which leaves the stop rule as it is.
    trace (a list): receives each step's mask uint8 [V] (1 = valid)."""
    ctx = get_ctx(v_rgb.device.index)
    V, n = v_rgb.shape[0], int(v_idx.shape[0])
    cur = _f(v_rgb).clone()
    if n == 0 or max_iters <= 0:
        return cur, 0
    idx = _i(v_idx.to(I32).contiguous())
    assert tuple(rowptr.shape) == (V + 1,), "rowptr is [V + 1]"      # the range of v_idx is the caller's to check (inpainting_vertex_color does, once)
    mask = torch.ones(V, dtype=U8, device=cur.device)
    mask[idx.long()] = 0
    nxt, mask_nxt = cur.clone(), mask.clone()
    counter = torch.zeros(1, dtype=I32, device=cur.device)
    count, steps = 0, 0
    for _ in range(int(max_iters)):
        ctx.check(ctx.lib.utx_vertex_inpaint_step(ctx.handle, ptr(_i(rowptr)), ptr(_i(col)), ptr(idx), n, ptr(cur), ptr(mask), ptr(nxt), ptr(mask_nxt), ptr(counter),
                                                  ctx.stream()))
        cur, nxt, mask, mask_nxt = nxt, cur, mask_nxt, mask
        steps += 1
        if trace is not None:
            trace.append(mask.clone())
        now = int(counter.item())
        if now <= count:
            break
        count = now
    return cur, steps


# ---- the blended UV texture bake (uv_bake.hip): project_uv_texture / remapping_uv_texture / uv_dilation of the reference

def uv_bake(rast2d, faces, face_mask, v_ndc, images, wmap, rast_view, map_Kd, weights, use_alpha=True, epilogue=None):
    """utx_uv_bake: rast2d [Th,Tw,4] (the atlas raster), faces [F,3] int32, face_mask uint8 [B,F] (visible_faces_*), v_ndc [B,V,2], images [B,4,R,R] rgba
    (planar, as given), wmap [B,R,R,2] (view_weight_maps), rast_view [B,R,R,4] (the views rasterised at R), map_Kd [Th,Tw,4], weights [B] ->
    (acc [Th,Tw,4], wacc [Th,Tw,1]): project_uv_texture's sum over the views (:479-505) in index order, in one launch, without the [B,R,R,6] map, the
    [B,Th,Tw,6] map_attr and the [B,Th,Tw,2] uv of the composition uv_project + elementwise steps, to which it is bit-identical.  epilogue =
    dict(overlay_confidence, blending (None | 'soft' | 'hard'), blending_confidence, inpainting_confidence): the same launch also applies
    remapping_uv_texture's overlay and blending (:205-217) and returns (acc, wacc, blended [Th,Tw,4], inpaint_mask uint8 [Th,Tw] = wacc <=
    inpainting_confidence on the texels the atlas raster covers)."""
    assert rast2d.dim() == 3 and rast2d.shape[2] == 4 and faces.dim() == 2 and faces.shape[1] == 3, "rast2d is [Th, Tw, 4], faces [F, 3]"
    Th, Tw = rast2d.shape[:2]
    F = faces.shape[0]
    if face_mask.dim() != 2 or face_mask.shape[1] != F or face_mask.shape[0] < 1:
        raise ValueError("uv_bake: face_mask is %s, expected [B >= 1, F = %d]" % (tuple(face_mask.shape), F))
    B = face_mask.shape[0]
    if v_ndc.dim() != 3 or v_ndc.shape[0] != B or v_ndc.shape[2] != 2 or v_ndc.shape[1] < 1:
        raise ValueError("uv_bake: v_ndc is %s, expected [B = %d, V, 2]" % (tuple(v_ndc.shape), B))
    V = v_ndc.shape[1]
    if images.dim() != 4 or images.shape[0] != B or images.shape[1] != 4 or images.shape[2] != images.shape[3] or images.shape[2] < 1:
        raise ValueError("uv_bake: images is %s, expected [B = %d, 4, R, R]" % (tuple(images.shape), B))
    R = images.shape[2]
    if tuple(wmap.shape) != (B, R, R, 2) or tuple(rast_view.shape) != (B, R, R, 4):
        raise ValueError("uv_bake: wmap is %s and rast_view %s, expected %s and %s" % (tuple(wmap.shape), tuple(rast_view.shape), (B, R, R, 2), (B, R, R, 4)))
    if tuple(map_Kd.shape) != (Th, Tw, 4) or tuple(weights.shape) != (B,):
        raise ValueError("uv_bake: map_Kd is %s and weights %s, expected %s and %s" % (tuple(map_Kd.shape), tuple(weights.shape), (Th, Tw, 4), (B,)))
    args = _epilogue_args(epilogue, "uv_bake")
    dev = rast2d.device
    ctx = get_ctx(dev.index)
    acc = torch.empty(Th, Tw, 4, dtype=F32, device=dev)
    wacc = torch.empty(Th, Tw, 1, dtype=F32, device=dev)
    blended = torch.empty(Th, Tw, 4, dtype=F32, device=dev) if epilogue is not None else None
    mask = torch.empty(Th, Tw, dtype=U8, device=dev) if epilogue is not None else None
    ctx.check(ctx.lib.utx_uv_bake(ctx.handle, ptr(_f(rast2d)), ptr(_i(faces)), F, ptr(_u8(face_mask)), ptr(_f(v_ndc)), V, B, Th, Tw, ptr(_f(images)), ptr(_f(wmap)),
                                  ptr(_f(rast_view)), R, ptr(_f(map_Kd)), ptr(_f(weights)), int(bool(use_alpha)), ptr(acc), ptr(wacc), int(epilogue is not None),
                                  *args, ptr(blended), ptr(mask), ctx.stream()))
    return (acc, wacc) if epilogue is None else (acc, wacc, blended, mask)


def uv_dilation(map_Kd, valid, max_iters=-1, trace=None):
    """uv_dilation (uv_dilation.py:33-50) on one image: map_Kd [H,W,C] (1 <= C <= 16), valid uint8 [H,W] (1 = keep, 0 = fill) -> (filled [H,W,C], number of
    steps).  One utx_uv_dilation_step launch per step, colour and mask double-buffered; after each step the host reads the 4-byte count of texels that are
    still invalid and stops at 0 (the reference's `prod() > 0`), at max_iters > 0, or when a step did not lower the count -- the one departure: with no
    valid texel in reach the reference loops forever, here the texels out of reach keep their colour.  A last launch clamps the whole map to [0, 1],
    also after zero steps.  trace (a list): receives each step's (colour, mask) clones."""
    assert map_Kd.dim() == 3 and tuple(valid.shape) == tuple(map_Kd.shape[:2]), "map_Kd is [H, W, C], valid [H, W]"
    H, W, Cc = map_Kd.shape
    if not 1 <= Cc <= 16:
        raise ValueError("uv_dilation: %d channels, 1 to 16 are built" % Cc)
    ctx = get_ctx(map_Kd.device.index)
    cur, mask = _f(map_Kd), _u8(valid)
    out = torch.empty_like(cur)
    steps = 0
    if H * W == 0:
        return out, steps
    bufs = [torch.empty_like(cur), torch.empty_like(cur)]
    masks = [torch.empty_like(mask), torch.empty_like(mask)]
    counter = torch.zeros(1, dtype=I32, device=cur.device)
    count = H * W - int(torch.count_nonzero(mask).item())
    while count > 0 and not (max_iters > 0 and steps >= max_iters):
        nxt, mask_nxt = bufs[steps & 1], masks[steps & 1]
        ctx.check(ctx.lib.utx_uv_dilation_step(ctx.handle, ptr(cur), ptr(mask), H, W, Cc, 0, ptr(nxt), ptr(mask_nxt), ptr(counter), ctx.stream()))
        cur, mask = nxt, mask_nxt
        steps += 1
        if trace is not None:
            trace.append((cur.clone(), mask.clone()))
        now = int(counter.item())
        if now >= count:
            break
        count = now
    ctx.check(ctx.lib.utx_uv_dilation_step(ctx.handle, ptr(cur), None, H, W, Cc, 1, ptr(out), None, None, ctx.stream()))
    return out, steps


# ---- the scattered-sample UV bake (global_bake.hip): global_inverse_rendering of the reference

KNN_INPAINT_K_MAX = 32      # utx_knn's and utx_knn_inpaint_step's cap


def _cos_threshold(degrees):
    """(use, cos) of an angle threshold in degrees, None = off; the cosine is rounded to float32, as the reference's comparison with a float32 tensor does"""
    return (0, 0.0) if degrees is None else (1, float(np.float32(math.cos(math.radians(float(degrees))))))


def view_samples(rast, faces, v_uv, v_pos_cam, v_nrm_cam, exclude_boundary=True, normal_angle_degree_threshold=None, ray_angle_degree_threshold=None,
                 image_mask=None):
    """utx_view_samples: rast [B,H,W,4] (the views' rasters), faces [F,3] int32, v_uv [V,2] in [-1,1], v_pos_cam / v_nrm_cam [B,V,3] (_camera_arrays: camera-space
    positions, NOT normalised, and normalised camera-space normals) -> (tex_to_pos [B,H,W,2], tex_to_pos_cam [B,H,W,6], mask uint8 [B,H,W]) of
    global_inverse_rendering (renderer_base.py:624-654) in one launch: the pixel's UV, the interpolation of the per-vertex normalised position direction and
    normal, and the sample mask -- coverage, the four torch.roll neighbours (wrapping round the edge), the two optional angle thresholds in degrees and the
    optional image_mask [B,H,W] (or [B,H,W,1]; non-zero = keep)."""
    if rast.dim() != 4 or rast.shape[3] != 4 or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError("view_samples: rast is %s and faces %s, expected [B, H, W, 4] and [F >= 1, 3]" % (tuple(rast.shape), tuple(faces.shape)))
    B, H, W = rast.shape[:3]
    if v_uv.dim() != 2 or v_uv.shape[1] != 2 or v_uv.shape[0] < 1:
        raise ValueError("view_samples: v_uv is %s, expected [V >= 1, 2]" % (tuple(v_uv.shape),))
    V = v_uv.shape[0]
    for name, a in (("v_pos_cam", v_pos_cam), ("v_nrm_cam", v_nrm_cam)):
        if B > 0 and (a is None or tuple(a.shape) != (B, V, 3)):
            raise ValueError("view_samples: %s is %s, expected %s" % (name, None if a is None else tuple(a.shape), (B, V, 3)))
    dev = rast.device
    if image_mask is not None:
        image_mask = torch.as_tensor(image_mask).to(dev)
        if image_mask.numel() != B * H * W:
            raise ValueError("view_samples: image_mask is %s, expected %s" % (tuple(image_mask.shape), (B, H, W)))
        image_mask = (image_mask.reshape(B, H, W) != 0).to(U8).contiguous()
    use_n, cos_n = _cos_threshold(normal_angle_degree_threshold)
    use_r, cos_r = _cos_threshold(ray_angle_degree_threshold)
    tex_to_pos = torch.empty(B, H, W, 2, dtype=F32, device=dev)
    tex_to_pos_cam = torch.empty(B, H, W, 6, dtype=F32, device=dev)
    mask = torch.empty(B, H, W, dtype=U8, device=dev)
    if B * H * W == 0:
        return tex_to_pos, tex_to_pos_cam, mask
    ctx = get_ctx(dev.index)
    ctx.check(ctx.lib.utx_view_samples(ctx.handle, ptr(_f(rast)), ptr(_i(faces)), faces.shape[0], ptr(_f(v_uv)), ptr(_f(v_pos_cam)), ptr(_f(v_nrm_cam)), V, B, H, W,
                                       int(bool(exclude_boundary)), use_n, cos_n, use_r, cos_r, ptr(image_mask) if image_mask is not None else None,
                                       ptr(tex_to_pos), ptr(tex_to_pos_cam), ptr(mask), ctx.stream()))
    return tex_to_pos, tex_to_pos_cam, mask


def knn_inpaint(idx, d2, nrm, col, pending, n_iters_max=1000, trace=None):
    """The propagation loop of global_inverse_rendering (renderer_base.py:702-722) on M points: idx int32 / d2 [M,k] (knn_gather(pos, pos, k, want_index=True)),
    nrm [M,3], col [M,C] (1 <= C <= 16), pending uint8 [M] (non-zero: to fill) -> (col, pending, steps).  One utx_knn_inpaint_step launch per step, colour and
    flag double-buffered; after each launch the host reads the 4-byte count of points it filled and stops at 0 (that launch changed nothing and is not a
    step) or after n_iters_max steps.  Points that never qualify stay pending with the colour they came with.  trace (a list): receives each step's pending
    flags (a clone)."""
    if idx.dim() != 2 or tuple(d2.shape) != tuple(idx.shape):
        raise ValueError("knn_inpaint: idx is %s and d2 %s, expected [M, k] both" % (tuple(idx.shape), tuple(d2.shape)))
    M, k = idx.shape
    if not 1 <= k <= KNN_INPAINT_K_MAX:
        raise ValueError("knn_inpaint: %d neighbours, 1 to %d are built" % (k, KNN_INPAINT_K_MAX))
    if col.dim() != 2 or col.shape[0] != M or not 1 <= col.shape[1] <= CHANNELS_MAX:
        raise ValueError("knn_inpaint: col is %s, expected [M = %d, 1 <= C <= %d]" % (tuple(col.shape), M, CHANNELS_MAX))
    if tuple(nrm.shape) != (M, 3) or tuple(pending.shape) != (M,):
        raise ValueError("knn_inpaint: nrm is %s and pending %s, expected %s and %s" % (tuple(nrm.shape), tuple(pending.shape), (M, 3), (M,)))
    Cc = col.shape[1]
    cur, pend = _f(col).clone(), _u8(pending).clone()
    steps = 0
    if M == 0 or n_iters_max <= 0:
        return cur, pend, steps
    ctx = get_ctx(col.device.index)
    nxt, pend_nxt = torch.empty_like(cur), torch.empty_like(pend)
    counter = torch.zeros(1, dtype=I32, device=col.device)
    p_idx, p_d2, p_nrm = ptr(_i(idx)), ptr(_f(d2)), ptr(_f(nrm))      # checked once: the lists do not change over the steps
    while steps < int(n_iters_max):
        ctx.check(ctx.lib.utx_knn_inpaint_step(ctx.handle, p_idx, p_d2, p_nrm, ptr(cur), ptr(pend), M, k, Cc, ptr(nxt), ptr(pend_nxt), ptr(counter), ctx.stream()))
        if int(counter.item()) == 0:
            break
        cur, nxt, pend, pend_nxt = nxt, cur, pend_nxt, pend
        steps += 1
        if trace is not None:
            trace.append(pend.clone())
    return cur, pend, steps


# ---- Poisson image fusion (image_fusion.hip): image_fusion of the reference; the rule is DESIGN 8 "Poisson image fusion"

MASK_MORPH_MAX = 31      # utx_mask_morph's cap on the box size


def mask_morph(mask, n):
    """mask uint8 [H,W]; n > 0: grey erosion over an n x n box, n < 0: grey dilation over |n| x |n| (offsets -(|n| // 2) .. |n| - 1 - |n| // 2, taps outside the
    image left out), n = 0: a copy.  Two separable launches (utx_mask_morph)."""
    n = int(n)
    if abs(n) > MASK_MORPH_MAX:
        raise ValueError("mask_morph: a box of %d, at most %d is built" % (abs(n), MASK_MORPH_MAX))
    if mask.dim() != 2:
        raise ValueError("mask_morph: mask is %s, expected [H, W]" % (tuple(mask.shape),))
    H, W = mask.shape
    if n == 0 or H * W == 0:
        return _u8(mask).clone()
    ctx = get_ctx(mask.device.index)
    tmp, out = torch.empty_like(mask), torch.empty_like(mask)
    ctx.check(ctx.lib.utx_mask_morph(ctx.handle, ptr(_u8(mask)), H, W, n, ptr(tmp), ptr(out), ctx.stream()))
    return out


def mask_bbox(mask):
    """(x1, y1, w, h): the tight bounding rectangle of mask > 0 (uint8 [H,W]), zeros for an empty mask.  One reduction and a 16-byte read-back (utx_mask_bbox)."""
    H, W = mask.shape
    if H * W == 0:
        return 0, 0, 0, 0
    ctx = get_ctx(mask.device.index)
    rect = torch.empty(4, dtype=I32, device=mask.device)
    ctx.check(ctx.lib.utx_mask_bbox(ctx.handle, ptr(_u8(mask)), H, W, ptr(rect), ctx.stream()))
    return tuple(int(v) for v in rect.cpu().tolist())


def image_fusion_u8(src_u8, dst_u8, mask_u8, n_erode_pix=0, return_float=False, cycles=0):
    """Poisson fusion of one image: src_u8, dst_u8 uint8 [H,W,3], mask_u8 uint8 [H,W] -> uint8 [H,W,3] (with return_float=True also the unrounded float32 result).
    The mask is resized by n_erode_pix (mask_morph), its bounding rectangle read back (the one host round trip: it sizes the multigrid levels), and
    utx_image_fusion solves for the correction on the rectangle's interior with a fixed number of V-cycles (cycles = 0: the library's count for the size)."""
    if src_u8.dim() != 3 or src_u8.shape[-1] != 3 or tuple(dst_u8.shape) != tuple(src_u8.shape) or tuple(mask_u8.shape) != tuple(src_u8.shape[:2]):
        raise ValueError("image_fusion_u8: src %s, dst %s, mask %s; expected [H, W, 3], [H, W, 3], [H, W]" %
                         (tuple(src_u8.shape), tuple(dst_u8.shape), tuple(mask_u8.shape)))
    H, W = mask_u8.shape
    out = torch.empty_like(_u8(dst_u8))
    out_f = torch.empty(H, W, 3, dtype=F32, device=out.device) if return_float else None
    if H * W == 0:
        return (out, out_f) if return_float else out
    ctx = get_ctx(src_u8.device.index)
    mask = mask_morph(mask_u8, n_erode_pix) if n_erode_pix else _u8(mask_u8)
    x1, y1, w, h = mask_bbox(mask)
    wb = int(ctx.lib.utx_image_fusion_workspace_bytes(w, h))
    work = torch.empty(max(wb, 4), dtype=U8, device=out.device)
    ctx.check(ctx.lib.utx_image_fusion(ctx.handle, ptr(_u8(src_u8)), ptr(_u8(dst_u8)), ptr(mask), H, W, x1, y1, w, h, int(cycles), ptr(out), ptr(out_f), ptr(work),
                                       wb, ctx.stream()))
    return (out, out_f) if return_float else out


# ---- Telea inpainting (inpaint.hip): cv2.inpaint(INPAINT_TELEA) of the reference; the rule is DESIGN 8 "Telea inpainting"

INPAINT_RADIUS_MAX = 8      # utx_inpaint_telea_step's cap on the radius
INPAINT_SIDE_MAX = 16384      # ... and on the image's sides (the squared distances stay inside int32)
INPAINT_NONE = 2147483647      # the distance where the whole image is a hole
INPAINT_READBACK = 4      # sweeps between two read-backs of the 4-byte counter (DESIGN 8 "Telea inpainting": measured at 1, 4 and 16)


def _inpaint_shape(who, H, W):
    if H > INPAINT_SIDE_MAX or W > INPAINT_SIDE_MAX:
        raise ValueError("%s: an image of %d x %d, sides up to %d are built" % (who, H, W, INPAINT_SIDE_MAX))


def inpaint_distance(hole):
    """hole uint8 [H,W] (non-zero: fill) -> int32 [H,W]: the exact squared Euclidean distance of every hole pixel to the nearest pixel outside the hole, 0 outside
    the hole, INPAINT_NONE everywhere when the whole image is a hole.  Two launches (utx_inpaint_distance): a column scan, then a per-pixel minimum over the row."""
    if hole.dim() != 2:
        raise ValueError("inpaint_distance: hole is %s, expected [H, W]" % (tuple(hole.shape),))
    H, W = hole.shape
    _inpaint_shape("inpaint_distance", H, W)
    d2 = torch.empty(H, W, dtype=I32, device=hole.device)
    if H * W == 0:
        return d2
    ctx = get_ctx(hole.device.index)
    tmp = torch.empty_like(d2)
    ctx.check(ctx.lib.utx_inpaint_distance(ctx.handle, ptr(_u8(hole)), H, W, ptr(tmp), ptr(d2), ctx.stream()))
    return d2


def inpaint_telea(img_u8, hole_u8, radius=1, return_float=False, trace=None, readback=None):
    """Telea inpainting of one image: img_u8 uint8 [H,W,C] (1 <= C <= 4), hole_u8 uint8 [H,W] (non-zero: fill), radius 1 .. 8 (<= 0 means 1, as OpenCV clamps
    the reference's -1) -> (uint8 [H,W,C], sweeps), with return_float=True (uint8, float32 [H,W,C] unrounded and unclamped, sweeps).  The distance map
    (inpaint_distance), then one utx_inpaint_telea_step launch per sweep on a float32 working image, colour and done flags double-buffered; every `readback`
    sweeps (None: INPAINT_READBACK) the host reads the 4-byte count of pixels computed since the last read and stops once every hole pixel is done, so up to
    readback - 1 sweeps that change nothing may be launched -- the result does not depend on it.  utx_inpaint_finish rounds once at the end.  An empty image,
    an empty hole and an all-hole image return a copy and 0 sweeps.  trace (a list): receives each sweep's done flags (a clone)."""
    if img_u8.dim() != 3 or not 1 <= img_u8.shape[2] <= 4 or tuple(hole_u8.shape) != tuple(img_u8.shape[:2]):
        raise ValueError("inpaint_telea: img is %s and hole %s, expected [H, W, 1 <= C <= 4] and [H, W]" % (tuple(img_u8.shape), tuple(hole_u8.shape)))
    if img_u8.dtype != U8:
        raise ValueError("inpaint_telea: img is %s, expected uint8" % img_u8.dtype)
    radius = max(int(radius), 1)
    if radius > INPAINT_RADIUS_MAX:
        raise ValueError("inpaint_telea: a radius of %d, at most %d is built" % (radius, INPAINT_RADIUS_MAX))
    k = INPAINT_READBACK if readback is None else int(readback)
    if k < 1:
        raise ValueError("inpaint_telea: readback is %d, expected >= 1" % k)
    H, W, Cc = img_u8.shape
    _inpaint_shape("inpaint_telea", H, W)
    img = img_u8.contiguous()
    pending = int(torch.count_nonzero(hole_u8).item()) if H * W else 0
    if pending == 0 or pending == H * W:      # nothing to fill, or nothing to fill from
        out = img.clone()
        return (out, out.to(F32), 0) if return_float else (out, 0)
    ctx = get_ctx(img.device.index)
    hole = _u8(hole_u8)
    d2 = inpaint_distance(hole)
    cur = img.to(F32)
    nxt = cur.clone()      # a sweep writes hole pixels only: both buffers hold the image outside the hole
    done = (hole == 0).to(U8)
    done_nxt = done.clone()
    counter = torch.zeros(1, dtype=I32, device=img.device)
    p_d2 = ptr(d2)
    sweeps = 0
    while pending > 0:
        for _ in range(k):
            ctx.check(ctx.lib.utx_inpaint_telea_step(ctx.handle, ptr(cur), ptr(done), p_d2, H, W, Cc, radius, ptr(nxt), ptr(done_nxt), ptr(counter), ctx.stream()))
            cur, nxt, done, done_nxt = nxt, cur, done_nxt, done
            sweeps += 1
            if trace is not None:
                trace.append(done.clone())
        filled = int(counter.item())
        counter.zero_()
        if filled == 0:
            raise RuntimeError("inpaint_telea: %d sweeps filled nothing with %d pixels pending" % (k, pending))
        pending -= filled
    out = torch.empty_like(img)
    out_f = torch.empty(H, W, Cc, dtype=F32, device=img.device) if return_float else None
    ctx.check(ctx.lib.utx_inpaint_finish(ctx.handle, ptr(cur), H, W, Cc, ptr(out), ptr(out_f), ctx.stream()))
    return (out, out_f, sweeps) if return_float else (out, sweeps)


# ---- sliced optimal-transport colour transfer and its regulariser (color_transfer.hip): DESIGN 8 "Colour transfer"

COLOR_TRANSFER_N_MAX = 1 << 30      # utx_color_transfer_ot's bound on the pixel count (exclusive)
BILATERAL_RADIUS_MAX = 27      # utx_bilateral_filter's cap on the radius: the 16 x 16 tile with its halo, 3 channels, stays within 64 KiB of LDS
BILATERAL_SIDE_MAX = 32768      # ... and on the image's sides


def _same_cuda_f32(who, **tensors):
    first = next(iter(tensors.values()))
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != first.device:
            raise ValueError("%s: %s is expected on one CUDA device with the other operands" % (who, name))
        if t.dtype != F32:
            raise ValueError("%s: %s is %s, expected float32" % (who, name, t.dtype))


def color_transfer_ot(src, dst, dirs, steps, batch_size):
    """The solver loop of sliced optimal-transport colour transfer (utx_color_transfer_ot): src, dst float32 [..., C] of one shape (1 <= C <= 4, 1 <= N < 2^30
    pixels), dirs float32 [steps * batch_size, C] on the device (unit directions, one per step and batch in that order) -> src's shape.  Per step, for each batch
    in order: both images projected onto the direction, the projections sorted (a stable radix sort on the total order of the bit patterns: -0 before +0, equal
    source projections in ascending pixel order), every source pixel's advect increased by the difference of the equally ranked projections times the direction;
    then src += advect / batch_size.  One stream, no read-back; steps = 0 returns a copy.  Non-finite pixels are not looked for: a check would cost a read-back."""
    who = "color_transfer_ot"
    steps, batch_size = int(steps), int(batch_size)
    if steps < 0 or batch_size < 1:
        raise ValueError("%s: steps is %d and batch_size %d, expected steps >= 0 and batch_size >= 1" % (who, steps, batch_size))
    _same_cuda_f32(who, src=src, dst=dst, dirs=dirs)
    if src.dim() < 1 or tuple(dst.shape) != tuple(src.shape):
        raise ValueError("%s: src is %s and dst %s, expected one shape [..., C]" % (who, tuple(src.shape), tuple(dst.shape)))
    Cc = src.shape[-1]
    if not 1 <= Cc <= 4:
        raise ValueError("%s: %d channels, 1 .. 4 are built" % (who, Cc))
    N = src.numel() // Cc
    if not 1 <= N < COLOR_TRANSFER_N_MAX:
        raise ValueError("%s: %d pixels, 1 .. 2^30 - 1 are built" % (who, N))
    if tuple(dirs.shape) != (steps * batch_size, Cc):
        raise ValueError("%s: dirs is %s, expected [steps * batch_size, C] = [%d, %d]" % (who, tuple(dirs.shape), steps * batch_size, Cc))
    ctx = get_ctx(src.device.index)
    s, d, dd = src.contiguous(), dst.contiguous(), dirs.contiguous()
    out = torch.empty_like(s)
    wb = int(ctx.lib.utx_color_transfer_ot_workspace_bytes(N, Cc)) if steps else 0
    work = torch.empty(max(wb, 4), dtype=U8, device=src.device)
    ctx.check(ctx.lib.utx_color_transfer_ot(ctx.handle, ptr(s), ptr(d), ptr(dd) if steps else None, N, Cc, steps, batch_size, ptr(out), ptr(work), wb, ctx.stream()))
    return out


def bilateral_radius(sigma_space):
    """the window radius of cv2.bilateralFilter with d = 0: max(1, rint(1.5 sigma_space)), halves to even"""
    return max(1, int(np.rint(1.5 * float(sigma_space))))


def bilateral_space_weights(sigma_space):
    """float32 [r + 1, r + 1], indexed [|dy|, |dx|]: exp(-(dx^2 + dy^2) / (2 sigma_space^2)) computed in float64 on the host and rounded once"""
    r = bilateral_radius(sigma_space)
    a = np.arange(r + 1, dtype=np.float64)
    return np.exp(-(a[:, None] ** 2 + a[None, :] ** 2) / (2.0 * float(sigma_space) ** 2)).astype(np.float32)


def bilateral_filter(img, sigma_color, sigma_space):
    """Joint bilateral filter of a float32 [H, W, C] image, C 1 or 3, by this library's rule on cv2.bilateralFilter(img, 0, sigma_color, sigma_space)'s documented
    parameters (utx_bilateral_filter; unpinned against OpenCV): radius bilateral_radius(sigma_space) <= BILATERAL_RADIUS_MAX, circular support, space weights
    bilateral_space_weights, colour weight exp(-(sum_c |delta_c|)^2 / (2 sigma_color^2)) on the L1 colour distance, reflect-101 borders, sum(w v) / sum(w)."""
    who = "bilateral_filter"
    _same_cuda_f32(who, img=img)
    if img.dim() != 3 or img.shape[2] not in (1, 3):
        raise ValueError("%s: img is %s, expected [H, W, C] with C 1 or 3" % (who, tuple(img.shape)))
    sigma_color, sigma_space = float(sigma_color), float(sigma_space)
    if not (sigma_color > 0.0 and sigma_space > 0.0 and math.isfinite(sigma_color) and math.isfinite(sigma_space)):
        raise ValueError("%s: sigma_color is %r and sigma_space %r, expected positive finite values" % (who, sigma_color, sigma_space))
    r = bilateral_radius(sigma_space)
    if r > BILATERAL_RADIUS_MAX:
        raise ValueError("%s: sigma_space %g asks for a radius of %d, at most BILATERAL_RADIUS_MAX = %d is built" % (who, sigma_space, r, BILATERAL_RADIUS_MAX))
    H, W, Cc = img.shape
    if not (1 <= H <= BILATERAL_SIDE_MAX and 1 <= W <= BILATERAL_SIDE_MAX and H * W < COLOR_TRANSFER_N_MAX):
        raise ValueError("%s: an image of %d x %d, sides of 1 .. %d and fewer than 2^30 pixels are built" % (who, H, W, BILATERAL_SIDE_MAX))
    ctx = get_ctx(img.device.index)
    ws = torch.from_numpy(bilateral_space_weights(sigma_space)).to(img.device)
    coef = float(np.float32(-0.5 / (sigma_color * sigma_color)))
    src = img.contiguous()
    out = torch.empty_like(src)
    ctx.check(ctx.lib.utx_bilateral_filter(ctx.handle, ptr(src), H, W, Cc, r, ptr(ws), coef, ptr(out), ctx.stream()))
    return out


# ---- silhouette antialiasing of screen-space buffers (antialias.hip): DESIGN 8 "Silhouette antialiasing"

def _antialias_operands(who, dtypes, **tensors):
    """type and dtype of the operands; the shapes follow, the devices come last (_antialias_devices), so that every shape error is raised without a device"""
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or t.dtype != dtypes[name]:
            raise ValueError("%s: %s is expected as a %s tensor" % (who, name, str(dtypes[name]).replace("torch.", "")))


def _antialias_devices(who, **tensors):
    first = next(iter(tensors.values()))
    for name, t in tensors.items():
        if not t.is_cuda or t.device != first.device:
            raise ValueError("%s: %s is expected on one CUDA device with the other operands" % (who, name))


def _antialias_geometry(who, rast, pos_clip, tri, opp):
    """the shapes of the analysis' operands -> (rast [B,H,W,4], pos_clip, tri, opp, per-view stride of pos_clip, squeeze the batch of the result?)"""
    _antialias_operands(who, dict(rast=F32, pos_clip=F32, tri=I32, opp=I32), rast=rast, pos_clip=pos_clip, tri=tri, opp=opp)
    if rast.dim() not in (3, 4) or rast.shape[-1] != 4 or min(rast.shape) < 1:
        raise ValueError("%s: rast is %s, expected [B, H, W, 4] or [H, W, 4] with no empty side" % (who, tuple(rast.shape)))
    squeeze = rast.dim() == 3
    rast4 = rast[None] if squeeze else rast
    B = rast4.shape[0]
    if pos_clip.dim() not in (2, 3) or pos_clip.shape[-1] != 4 or pos_clip.shape[-2] < 1 or (pos_clip.dim() == 3 and pos_clip.shape[0] != B):
        raise ValueError("%s: pos_clip is %s, expected [V, 4] or [B = %d, V, 4]" % (who, tuple(pos_clip.shape), B))
    if tri.dim() != 2 or tri.shape[1] != 3 or tri.shape[0] < 1 or tuple(opp.shape) != tuple(tri.shape):
        raise ValueError("%s: tri is %s and opp %s, expected [F >= 1, 3] both" % (who, tuple(tri.shape), tuple(opp.shape)))
    _antialias_devices(who, rast=rast, pos_clip=pos_clip, tri=tri, opp=opp)
    V = pos_clip.shape[-2]
    return rast4.contiguous(), pos_clip.contiguous(), tri.contiguous(), opp.contiguous(), (4 * V if pos_clip.dim() == 3 else 0), squeeze


def antialias_weights(rast, pos_clip, tri, opp):
    """The geometry half of silhouette antialiasing (utx_antialias_analyze): rast [B,H,W,4] or [H,W,4] (ops.rasterize's records, one raster per view),
    pos_clip [B,V,4] or [V,4] (the clip-space vertices the rasters were made from; [V,4] is shared by the views), tri [F,3] int32, opp [F,3] int32
    (meshes.edge_opposites) -> weights float32 of rast's shape: per pixel (left, right, up, down), the share in [0, 0.5] of the difference to that
    neighbour that the pixel takes.  Non-zero only where a pair of neighbouring pixels shows two different triangles (or one and the background) and a
    silhouette edge of the nearer one crosses the segment between the two pixel centres nearer to the other pixel than to this one.  It depends on the
    geometry alone: compute it once per rasterisation and hand it to antialias_apply for every buffer."""
    who = "antialias_weights"
    rast4, pos, tri, opp, stride, squeeze = _antialias_geometry(who, rast, pos_clip, tri, opp)
    B, H, W = rast4.shape[:3]
    ctx = get_ctx(rast4.device.index)
    weights = torch.empty_like(rast4)
    ctx.check(ctx.lib.utx_antialias_analyze(ctx.handle, ptr(rast4), ptr(pos), stride, ptr(tri), ptr(opp), tri.shape[0], pos.shape[-2], B, H, W, ptr(weights),
                                            ctx.stream()))
    return weights[0] if squeeze else weights


def antialias_apply(color, weights):
    """The stencil half of silhouette antialiasing (utx_antialias_apply): color float32 [B,H,W,C] or [H,W,C], any C >= 1, weights [B,H,W,4] or [H,W,4]
    from antialias_weights -> out = (((color + k_left) + k_right) + k_up) + k_down per channel, k_n = w_n * (color[n] - color) where w_n != 0, in this
    order: a new tensor, bit-reproducible."""
    who = "antialias_apply"
    _antialias_operands(who, dict(color=F32, weights=F32), color=color, weights=weights)
    if color.dim() not in (3, 4) or min(color.shape) < 1:
        raise ValueError("%s: color is %s, expected [B, H, W, C] or [H, W, C] with no empty side" % (who, tuple(color.shape)))
    if weights.dim() != color.dim() or tuple(weights.shape) != tuple(color.shape[:-1]) + (4,):
        raise ValueError("%s: weights is %s, expected %s for a color of %s" % (who, tuple(weights.shape), tuple(color.shape[:-1]) + (4,), tuple(color.shape)))
    _antialias_devices(who, color=color, weights=weights)
    B, H, W, Cc = ((1,) + tuple(color.shape))[-4:]
    ctx = get_ctx(color.device.index)
    src, w = color.contiguous(), weights.contiguous()
    out = torch.empty_like(src)
    ctx.check(ctx.lib.utx_antialias_apply(ctx.handle, ptr(src), ptr(w), B, H, W, Cc, ptr(out), ctx.stream()))
    return out


def antialias(color, rast, pos_clip, tri, opp=None):
    """Silhouette antialiasing of one screen-space buffer, the forward pass of what the reference calls dr.antialias(color, rast, pos_clip, tri):
    antialias_apply(color, antialias_weights(rast, pos_clip, tri, opp)), bit-identical to the two calls.  opp=None computes the topology from tri on
    the host (meshes.edge_opposites): a caller with more than one buffer or call keeps opp, and the weights.  The rule is this library's, after Laine
    et al. 2020 section 3.5; nvdiffrast's samples are not pinned (DESIGN 8 "Silhouette antialiasing")."""
    who = "antialias"
    if opp is None:
        if not isinstance(tri, torch.Tensor) or tri.dtype != I32 or tri.dim() != 2 or tri.shape[1:] != (3,):
            raise ValueError("%s: tri is expected as an int32 tensor [F, 3]" % who)
        from . import meshes
        opp = torch.from_numpy(meshes.edge_opposites(tri.cpu().numpy())).to(tri.device)
    _antialias_operands(who, dict(color=F32, rast=F32), color=color, rast=rast)
    if color.dim() != rast.dim() or tuple(color.shape[:-1]) != tuple(rast.shape[:-1]):
        raise ValueError("%s: color is %s and rast %s, expected one screen" % (who, tuple(color.shape), tuple(rast.shape)))
    return antialias_apply(color, antialias_weights(rast, pos_clip, tri, opp))
