"""Blended multi-view UV texture bake: texture/reprojection/mesh_remapping.py of the reference, the atlas half, and its uv_dilation.

    project_uv_texture      (:430-505)  the views' colours accumulated per atlas texel with facing weights
    remapping_uv_texture    (:145-270)  ... then overlay, blending against the given atlas, inpainting of the unseen texels, outpainting of the rest
    remapping_uv_texture_v2 (:25-142)   the scattered-sample bake (NVDiffRendererInverse.global_inverse_rendering), then outpainting
    uv_dilation             (texture/reprojection/uv_dilation.py:33-50, step :80-92)  texel-space dilation

Names, argument names, argument order and defaults are the reference's.  `mesh` is what the inverse renderer holds: a renderer_inverse.DeviceMesh, or an
NVDiffRendererInverse whose mesh is set.  Tensors may live anywhere; results are float32 on the mesh's device.  Atlas row 0 is v = 0, as everywhere in
simple_inverse_rendering.

Three readings of the reference, recorded by the fixture (tests/golden/g21_uv_bake.npz):
  (a) map_Kd=None: the reference makes a 3-channel zero map, which :503 cannot broadcast against the 4-channel view colours (RuntimeError).  Here None is
      zeros [T,T,4] and no blending; a [T,T,3] map_Kd is given a zero fourth channel, which never reaches the returned rgb.
  (b) the alpha of :503 is the view's uv_alpha (visibility and coverage), not the image's alpha channel, which is only carried as channel 3 of the
      accumulator.
  (c) use_alpha=False: a texel whose uv lands off the view's coverage contributes texel [0, 0] of the view's image and weight maps
      (simple_inverse_rendering's rule for background=None).  Reproduced, not repaired.
One departure: uv_dilation stops when a step fills nothing more (the reference loops forever when no valid texel is in reach).

Refused, never dropped (NotImplementedError): visualize=True (cv2 debug images) everywhere; in remapping_uv_texture also use_cv_inpainting=True -- the
reference's DEFAULT, cv2.inpaint (Telea): pass use_cv_inpainting=False --, use_cv_outpainting=True and blending_type='poisson', whose refusals its tests pin.

Those three branches run under new names:
    uv_dilation_cv          (uv_dilation.py:15-29)  the reference's quantisation around ops.inpaint_telea (csrc/inpaint.hip): Telea inpainting on the device,
                            by this library's own rule (DESIGN 8 "Telea inpainting"), not OpenCV's heap order [3p]
    remapping_uv_texture_cv the reference's signature and defaults with use_cv_inpainting, use_cv_outpainting and blending_type='poisson' running; the 'poisson'
                            branch (:213) is the composition
                                acc, wacc = project_uv_texture(mesh, c2ws, intrinsics, images, map_Kd, weights)
                                overlay = torch.where(wacc > overlay_confidence, acc / wacc, acc)
                                rgb = image_fusion(overlay[None, ..., :3], map_Kd[None, ..., :3], (wacc > blending_confidence).float()[None])[0]
                            With the cv flags off and 'soft' / 'hard' it returns remapping_uv_texture's bytes (one shared body).
remapping_uv_texture_v2 and initial_map_Kd_with_v_rgb keep refusing use_cv_outpainting=True."""
import numpy as np
import torch

from . import ops
from .remapping import _refuse_visualize, _renderer, default_weights
from .renderer_inverse import _reads_vertex_normals


def _bake(who, mesh, c2ws, intrinsics, images, map_Kd, weights, use_alpha, render_size, texture_size, perspective, epilogue):
    r = _renderer(mesh)
    m, dev = r.pbr_mesh, r.device
    c2ws = torch.as_tensor(c2ws, dtype=torch.float32).cpu()
    if c2ws.dim() != 3 or tuple(c2ws.shape[1:]) != (4, 4) or c2ws.shape[0] < 1:
        raise ValueError("%s: c2ws is %s, expected [B >= 1, 4, 4]" % (who, tuple(c2ws.shape)))
    B = c2ws.shape[0]
    if isinstance(render_size, (tuple, list)) or isinstance(texture_size, (tuple, list)):
        raise ValueError("%s: render_size and texture_size are one number each" % who)
    R, T = int(render_size), int(texture_size)
    if R < 2 or T < 1:
        raise ValueError("%s: render_size %d (>= 2) and texture_size %d (>= 1)" % (who, R, T))
    intrinsics = torch.as_tensor(intrinsics, dtype=torch.float32).cpu().expand(B, -1, -1)
    images = torch.as_tensor(images, dtype=torch.float32).to(dev).contiguous()
    if tuple(images.shape) != (B, 4, R, R):      # the reference concatenates them with the weight maps rendered at render_size (:480)
        raise ValueError("%s: images is %s, expected [%d, 4, render_size = %d, %d] rgba" % (who, tuple(images.shape), B, R, R))
    map_Kd = torch.as_tensor(map_Kd, dtype=torch.float32).to(dev)
    if map_Kd.dim() != 3 or tuple(map_Kd.shape[:2]) != (T, T) or map_Kd.shape[2] not in (3, 4):
        raise ValueError("%s: map_Kd is %s, expected [%d, %d, 4] (or 3 channels)" % (who, tuple(map_Kd.shape), T, T))
    if map_Kd.shape[2] == 3:
        map_Kd = torch.cat([map_Kd, torch.zeros_like(map_Kd[..., :1])], dim=-1)
    map_Kd = map_Kd.contiguous()
    weights = torch.as_tensor(weights, dtype=torch.float32).to(dev).contiguous()
    if tuple(weights.shape) != (B,):
        raise ValueError("%s: weights is %s, expected [%d]" % (who, tuple(weights.shape), B))
    # ONE rasterisation of the views: the weight maps and the coverage both read it
    _, c2ws_cpu, _, ndc, rast = r._view_raster(c2ws, intrinsics, R, perspective)
    want = ["cos_ray_normal"] + ([] if perspective else ["camera_normal"])
    g = ops.screen_gbuffer(rast, m.faces, m.vertices, v_nrm=m.vertex_normals if _reads_vertex_normals(want) else None, c2ws=c2ws_cpu, want=want)
    wmap = ops.view_weight_maps(g["cos_ray_normal"], None if perspective else g["camera_normal"], r=ops.weight_map_radius(R))
    rast2d = r._uv_raster(T, T)
    face_mask = r._visible_faces(c2ws, perspective, "rays", None, 0)      # simple_inverse_rendering(render_uv=True)'s default
    return rast2d, map_Kd, ops.uv_bake(rast2d, m.faces, face_mask, ndc, images, wmap, rast, map_Kd, weights, use_alpha=use_alpha, epilogue=epilogue)


def project_uv_texture(mesh, c2ws, intrinsics, images, map_Kd, weights, use_alpha=True, render_size=512, texture_size=1024, visualize=False, perspective=True):
    """c2ws [B,4,4], intrinsics [B,3,3] (or [3,3]), images [B,4,render_size,render_size] rgba, map_Kd [T,T,4], weights [B] ->
    (map_Kd_rgb_acc [T,T,4], map_Kd_weight_acc [T,T,1]).  Per view and texel: uv, uv_alpha (the face is seen by the view -- one ray per face, no erosion --
    and the view covers the pixel under uv) as simple_inverse_rendering(render_uv=True, render_map_attr=True) gives them; the image and the two weight maps
    (ops.view_weight_maps on the views rendered at render_size; orthographic: camera_normal.z) sampled bilinearly at uv; a = use_alpha ? uv_alpha : 1;
    weight = weights[b] * cos^4 * a * (1 - edge alpha); colour = (a * rgba + (1 - a) * map_Kd) * weight.  Both are summed over the views in index
    order, in one kernel launch (ops.uv_bake)."""
    _refuse_visualize("project_uv_texture", visualize)
    if map_Kd is None:
        raise ValueError("project_uv_texture: map_Kd is required, [texture_size, texture_size, 4]")
    return _bake("project_uv_texture", mesh, c2ws, intrinsics, images, map_Kd, weights, use_alpha, render_size, texture_size, perspective, None)[2]


def _remapping_uv_texture(who, cv, mesh, c2ws, intrinsics, images, map_Kd, weights, use_alpha, overlay_confidence, use_blending, blending_type,
                          blending_confidence, use_inpainting, use_cv_inpainting, inpainting_confidence, use_outpainting, use_cv_outpainting, render_size,
                          texture_size, visualize, perspective, return_stages):
    """the one body of remapping_uv_texture and remapping_uv_texture_cv; cv=False keeps the three refusals of the former"""
    _refuse_visualize(who, visualize)
    batch_size = torch.as_tensor(c2ws).shape[0]
    if weights is not None and len(weights) != batch_size:
        raise ValueError("size mismatch: length of weights should be %d but %d" % (batch_size, len(weights)))
    if blending_type not in ("poisson", "soft", "hard"):
        raise ValueError("value error: %s is not supported" % (blending_type,))
    if not cv:
        if blending_type == "poisson":
            raise NotImplementedError("remapping_uv_texture(blending_type='poisson') is not built: 'soft' or 'hard'")
        if use_inpainting and use_cv_inpainting:
            raise NotImplementedError("remapping_uv_texture(use_cv_inpainting=True) is not built (cv2.inpaint): pass use_cv_inpainting=False for uv_dilation")
        if use_outpainting and use_cv_outpainting:
            raise NotImplementedError("remapping_uv_texture(use_cv_outpainting=True) is not built (cv2.inpaint): the outpainting is pull_push")
    r = _renderer(mesh)
    T = int(texture_size)
    if map_Kd is None:
        map_Kd = torch.zeros(T, T, 4, dtype=torch.float32, device=r.device)
        use_blending = False
    if weights is None:
        weights = default_weights(batch_size)
    weights = torch.as_tensor(np.asarray(weights, dtype=np.float32))
    poisson = bool(use_blending) and blending_type == "poisson"      # the overlay stage alone comes from the launch; the fusion follows it (:213)
    epilogue = dict(overlay_confidence=overlay_confidence, blending=blending_type if use_blending and not poisson else None,
                    blending_confidence=blending_confidence, inpainting_confidence=inpainting_confidence)
    rast2d, kd4, (acc, wacc, blended, mask) = _bake(who, r, c2ws, intrinsics, images, map_Kd, weights, use_alpha, render_size, T, perspective, epilogue)
    covered = (rast2d[..., 3] > 0).to(torch.uint8).contiguous()      # compute_uv_mask: the coverage of the same raster
    rgb, steps = blended[..., :3].contiguous(), 0
    if poisson:
        from .image_fusion import image_fusion
        rgb = image_fusion(rgb[None], kd4[None, ..., :3], (wacc > blending_confidence).to(torch.float32)[None])[0].contiguous()
        blended = torch.cat([rgb, blended[..., 3:]], dim=-1)
    if use_inpainting:
        if use_cv_inpainting:
            rgb = uv_dilation_cv(rgb.permute(2, 0, 1)[None], mask[None, None] != 0)[0].permute(1, 2, 0).contiguous()
        else:
            rgb, steps = ops.uv_dilation(rgb, (1 - mask).contiguous())
    inpainted = rgb
    if use_outpainting:
        if use_cv_outpainting:
            rgb = uv_dilation_cv(rgb.permute(2, 0, 1)[None], (covered == 0)[None, None])[0].permute(1, 2, 0).contiguous()
        else:
            rgb = ops.pull_push(rgb, covered)
    out = torch.cat([rgb, covered[..., None].to(torch.float32)], dim=-1)
    if return_stages:
        return out, dict(map_Kd_rgb_acc=acc, map_Kd_weight_acc=wacc, blended=blended, inpaint_mask=mask, inpainted=inpainted, inpaint_steps=steps, map_Kd=out)
    return out


def remapping_uv_texture(mesh, c2ws, intrinsics, images, map_Kd=None, weights=None, use_alpha=True, overlay_confidence=0.2, use_blending=True,
                         blending_type="soft", blending_confidence=0.2, use_inpainting=True, use_cv_inpainting=True, inpainting_confidence=0.2,
                         use_outpainting=True, use_cv_outpainting=False, render_size=512, texture_size=1024, visualize=False, perspective=True,
                         return_stages=False):
    """project_uv_texture, then (:205-269): overlay -- the accumulated colour divided by the accumulated weight where that exceeds overlay_confidence;
    blending against map_Kd where the weight is at most blending_confidence ('soft': (map_Kd * (conf - w) + acc) / conf, 'hard': map_Kd); inpainting of
    the covered texels whose weight is at most inpainting_confidence (uv_dilation); outpainting of the texels the atlas does not cover (ops.pull_push);
    rgb with the atlas coverage as alpha.  map_Kd=None: zeros and no blending.  weights=None: the reference's table for 8 / 6 / 4 / 2 views, ones
    otherwise.  Returns [T,T,4]; with return_stages=True a dict of every stage as well (map_Kd_rgb_acc, map_Kd_weight_acc, blended, inpaint_mask,
    inpainted, inpaint_steps, map_Kd).  A weights of the wrong length and an unknown blending_type raise ValueError (the reference's two assertions);
    see the module docstring for what is refused -- remapping_uv_texture_cv runs those branches."""
    return _remapping_uv_texture("remapping_uv_texture", False, mesh, c2ws, intrinsics, images, map_Kd, weights, use_alpha, overlay_confidence, use_blending,
                                 blending_type, blending_confidence, use_inpainting, use_cv_inpainting, inpainting_confidence, use_outpainting,
                                 use_cv_outpainting, render_size, texture_size, visualize, perspective, return_stages)


def remapping_uv_texture_cv(mesh, c2ws, intrinsics, images, map_Kd=None, weights=None, use_alpha=True, overlay_confidence=0.2, use_blending=True,
                            blending_type="soft", blending_confidence=0.2, use_inpainting=True, use_cv_inpainting=True, inpainting_confidence=0.2,
                            use_outpainting=True, use_cv_outpainting=False, render_size=512, texture_size=1024, visualize=False, perspective=True,
                            return_stages=False):
    """remapping_uv_texture with the reference's signature and defaults and every branch but visualize=True running: use_cv_inpainting=True (the reference's
    default) fills the inpainting mask with uv_dilation_cv, use_cv_outpainting=True the texels the atlas does not cover, and blending_type='poisson' takes the
    overlay stage (the launch's epilogue with no blending) through image_fusion(overlay rgb, map_Kd rgb, weight > blending_confidence) (:213).  The `blended`
    stage of return_stages is the fused image then.  With use_cv_inpainting=False, use_cv_outpainting=False and 'soft' / 'hard' the result is
    remapping_uv_texture's, bit for bit: the two share one body."""
    return _remapping_uv_texture("remapping_uv_texture_cv", True, mesh, c2ws, intrinsics, images, map_Kd, weights, use_alpha, overlay_confidence, use_blending,
                                 blending_type, blending_confidence, use_inpainting, use_cv_inpainting, inpainting_confidence, use_outpainting,
                                 use_cv_outpainting, render_size, texture_size, visualize, perspective, return_stages)


def remapping_uv_texture_v2(mesh, c2ws, intrinsics, images, map_Kd=None, use_outpainting=True, use_cv_outpainting=False, render_size=512, texture_size=1024,
                            angle_degree_threshold=45.0, visualize=False, visualize_detail=False, perspective=True, grid_interpolate_mode="nearest"):
    """remapping_uv_texture_v2 (:25-142): images [B,4,render_size,render_size] rgba baked through global_inverse_rendering -- every view pixel a sample at its
    own UV, the texels some view sees take their nearest sample, the texels no view sees are filled along the surface (n_neighbors = 10, at most 1000
    steps) --, then outpainting of the texels the atlas does not cover (alpha <= 0.6; ops.pull_push) -> [T,T,4] = rgb and the atlas coverage.
    render_size above 768 resamples the images to 768 x 768 (F.interpolate, nearest) first, as the reference does.  angle_degree_threshold (None: off) is
    the ray-angle threshold of a perspective bake and the normal-angle threshold of an orthographic one.  map_Kd is ignored, as in the reference.
    grid_interpolate_mode is this build's one keyword: 'nearest' here, where the reference passes nothing and so runs its 'linear' (a scipy Delaunay
    interpolator on the host, not built; 'linear' and 'barycentric' raise NotImplementedError naming 'nearest').  Refused, never dropped
    (NotImplementedError): use_cv_outpainting=True, visualize=True, visualize_detail=True."""
    _refuse_visualize("remapping_uv_texture_v2", visualize)
    if visualize_detail:
        raise NotImplementedError("remapping_uv_texture_v2(visualize_detail=True) is not built: it writes cv2 debug images")
    if use_outpainting and use_cv_outpainting:
        raise NotImplementedError("remapping_uv_texture_v2(use_cv_outpainting=True) is not built (cv2.inpaint): the outpainting is pull_push")
    r = _renderer(mesh)
    if isinstance(render_size, (tuple, list)) or isinstance(texture_size, (tuple, list)):
        raise ValueError("remapping_uv_texture_v2: render_size and texture_size are one number each")
    R, T = int(render_size), int(texture_size)
    images = torch.as_tensor(images, dtype=torch.float32).to(r.device)
    B = torch.as_tensor(c2ws).shape[0]
    if tuple(images.shape) != (B, 4, R, R):
        raise ValueError("remapping_uv_texture_v2: images is %s, expected [%d, 4, render_size = %d, %d] rgba" % (tuple(images.shape), B, R, R))
    if R > 768:      # "before using a faster interpolation algorithm, downsample images to 768*768" (:44-47)
        images = torch.nn.functional.interpolate(images, (768, 768))
        R = 768
    intrinsics = torch.as_tensor(intrinsics, dtype=torch.float32).cpu().expand(B, -1, -1)
    thr = dict(ray_angle_degree_threshold=angle_degree_threshold) if perspective else dict(normal_angle_degree_threshold=angle_degree_threshold)
    ret = r.global_inverse_rendering(images.permute(0, 2, 3, 1).contiguous(), c2ws, intrinsics, R, T, grid_interpolate_mode=grid_interpolate_mode,
                                     perspective=perspective, **thr)
    rgb, alpha = ret["map_attr"][..., :3].contiguous(), ret["map_alpha"]
    if use_outpainting:
        rgb = ops.pull_push(rgb, (alpha[..., 0] > 0.6).to(torch.uint8).contiguous())
    return torch.cat([rgb, alpha], dim=-1)


def uv_dilation(map_Kd, map_mask, max_iters=-1, return_steps=False):
    """map_Kd [1,C,H,W] float32 (1 <= C <= 16), map_mask [1,1,H,W] (non-zero: the texels to fill) -> [1,C,H,W] clamped to [0, 1].  Each step gives every
    texel next to a texel of the other kind the average of its valid 3 x 3 neighbours -- valid border texels are averaged again, as in the reference --
    and makes a texel valid once it has a valid neighbour; the loop ends when no invalid texel is left, after max_iters > 0 steps, or when a step filled
    nothing (texels out of reach keep their colour; the reference loops forever).  A batch of more than one image is refused (NotImplementedError):
    the reference steps the whole batch until every image is full, which couples the images' step counts.  return_steps=True: (map, steps)."""
    map_Kd = torch.as_tensor(map_Kd, dtype=torch.float32)
    if not map_Kd.is_cuda:
        map_Kd = map_Kd.to("cuda")
    map_mask = torch.as_tensor(map_mask).to(map_Kd.device)
    if map_Kd.dim() != 4 or map_mask.dim() != 4 or tuple(map_mask.shape) != (map_Kd.shape[0], 1) + tuple(map_Kd.shape[2:]):
        raise ValueError("uv_dilation: map_Kd is %s and map_mask %s, expected [N, C, H, W] and [N, 1, H, W]" % (tuple(map_Kd.shape), tuple(map_mask.shape)))
    if map_Kd.shape[0] != 1:
        raise NotImplementedError("uv_dilation: a batch of %d images is not built: one image per call" % map_Kd.shape[0])
    out, steps = ops.uv_dilation(map_Kd[0].permute(1, 2, 0).contiguous(), (map_mask[0, 0] == 0).to(torch.uint8).contiguous(), max_iters=max_iters)
    out = out.permute(2, 0, 1)[None]
    return (out, steps) if return_steps else out


def uv_dilation_cv(map_Kd, map_mask, max_iters=-1):
    """uv_dilation_cv of the reference (uv_dilation.py:15-29): map_Kd [N,C,H,W] float (1 <= C <= 4), map_mask [N,1,H,W] bool (true: the texels to fill) ->
    [N,C,H,W] in map_Kd's dtype.  Each image is quantised as the reference does -- clamp(0, 1) * 255 truncated to uint8 --, filled on its own by
    ops.inpaint_telea with max_iters as the RADIUS, exactly as the reference passes it to cv2.inpaint (-1, its default, is clamped to 1), and divided by 255.
    The fill is this library's Telea rule (DESIGN 8 "Telea inpainting"), not OpenCV's heap order [3p].  A new tensor is returned; the reference writes into
    map_Kd as well."""
    map_Kd = torch.as_tensor(map_Kd)
    if not map_Kd.is_floating_point():
        raise ValueError("uv_dilation_cv: map_Kd is %s, a float tensor in [0, 1] is expected" % map_Kd.dtype)
    if not map_Kd.is_cuda:
        map_Kd = map_Kd.to("cuda")
    map_mask = torch.as_tensor(map_mask).to(map_Kd.device)
    if map_Kd.dim() != 4 or map_mask.dim() != 4 or tuple(map_mask.shape) != (map_Kd.shape[0], 1) + tuple(map_Kd.shape[2:]):
        raise ValueError("uv_dilation_cv: map_Kd is %s and map_mask %s, expected [N, C, H, W] and [N, 1, H, W]" % (tuple(map_Kd.shape), tuple(map_mask.shape)))
    if not 1 <= map_Kd.shape[1] <= 4:
        raise ValueError("uv_dilation_cv: %d channels, 1 to 4 are built" % map_Kd.shape[1])
    q = map_Kd.permute(0, 2, 3, 1).clamp(0, 1).mul(255).to(torch.uint8).contiguous()
    m = map_mask.to(torch.bool).permute(0, 2, 3, 1)[..., 0].to(torch.uint8).mul(255).contiguous()
    res = torch.empty_like(map_Kd)
    for i in range(map_Kd.shape[0]):
        out = ops.inpaint_telea(q[i], m[i], radius=max_iters)[0]
        res[i] = out.to(map_Kd.dtype).div(255).permute(2, 0, 1)
    return res
