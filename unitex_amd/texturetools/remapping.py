"""Vertex-colour bake from views: texture/reprojection/mesh_remapping.py of the reference, the vertex half.

    project_vertex_color        (:508-602)  the views' colours accumulated per vertex with facing weights
    remapping_vertex_color      (:273-350)  ... then overlay, blending against the given colours, inpainting of the unseen vertices
    inpainting_vertex_color     (:605-627)  Jacobi fill along the mesh graph (Mesh.laplacian, mesh/structure.py:743-774)
    initial_map_Kd_with_v_rgb   (:353-427)  the vertex colours as a first atlas

Names, argument names and defaults are the reference's.  `mesh` is what the inverse renderer holds: a renderer_inverse.DeviceMesh, or an
NVDiffRendererInverse whose mesh is set.  Tensors may live anywhere; results are float32 on the mesh's device.

reference_transform.  project_vertex_color (:565) transforms the vertices with c2ws[b] ITSELF before projecting them, while the visibility and the weight
maps of the same function are rendered with its inverse (the renderer's own world-to-camera matrices).  reference_transform=False (default) hands the
kernel the world-to-camera matrices, so a vertex reads its colour and its weight at the pixel it was rendered to; reference_transform=True hands it c2ws[b],
which is what the reference executes.  Both run the same kernel; both are pinned against the reference's arrays (tests/golden/g20_vertex_bake.npz; for
False the fixture maker wraps the reference's apply_transform to invert each matrix with the reference's own c2w_to_w2c).

Refused, never dropped: visualize=True everywhere (it writes cv2 debug images), use_pymeshlab=True and use_cv_outpainting=True (NotImplementedError).
remapping_uv_texture, project_uv_texture and uv_dilation live in remapping_uv.py."""
import numpy as np
import torch

from . import camera, ops
from .renderer_inverse import DeviceMesh, NVDiffRendererInverse

DEFAULT_WEIGHTS = {8: [2.0, 0.05, 0.2, 0.02, 1.0, 0.02, 0.2, 0.05], 6: [2.0, 0.05, 0.2, 1.0, 0.2, 0.05], 4: [2.0, 0.2, 1.0, 0.2], 2: [1.0, 1.0]}


def default_weights(batch_size):
    """the reference's per-view weight tables (:297-307): front and back views count most; any other view count weighs all views alike"""
    return list(DEFAULT_WEIGHTS.get(int(batch_size), [1.0] * int(batch_size)))


def _renderer(mesh):
    if isinstance(mesh, NVDiffRendererInverse):
        if mesh.pbr_mesh is None:
            raise ValueError("the renderer holds no mesh: update_from_file / update_from_arrays first")
        return mesh
    if isinstance(mesh, DeviceMesh):
        return NVDiffRendererInverse(device=mesh.device, pbr_mesh=mesh)
    raise TypeError("mesh is %s: a DeviceMesh or an NVDiffRendererInverse" % type(mesh).__name__)


def _refuse_visualize(who, visualize):
    if visualize:
        raise NotImplementedError("%s(visualize=True) is not built: it writes cv2 debug images" % who)


def _adjacency(m):
    """the mesh's CSR vertex adjacency, built once per DeviceMesh"""
    adj = getattr(m, "_vertex_adjacency", None)
    if adj is None:
        adj = m._vertex_adjacency = ops.vertex_adjacency(m.faces, m.vertices.shape[0])
    return adj


def _project(who, mesh, c2ws, intrinsics, images, v_rgb, weights, use_alpha, render_size, perspective, reference_transform, epilogue):
    r = _renderer(mesh)
    m, dev = r.pbr_mesh, r.device
    c2ws = torch.as_tensor(c2ws, dtype=torch.float32).cpu()
    if c2ws.dim() != 3 or tuple(c2ws.shape[1:]) != (4, 4) or c2ws.shape[0] < 1:
        raise ValueError("%s: c2ws is %s, expected [B >= 1, 4, 4]" % (who, tuple(c2ws.shape)))
    B, V = c2ws.shape[0], m.vertices.shape[0]
    intrinsics = torch.as_tensor(intrinsics, dtype=torch.float32).cpu().expand(B, -1, -1)
    images = torch.as_tensor(images, dtype=torch.float32).to(dev).contiguous()
    if images.dim() != 4 or images.shape[0] != B or images.shape[1] != 4 or min(images.shape) < 1:
        raise ValueError("%s: images is %s, expected [%d, 4, H, W] rgba" % (who, tuple(images.shape), B))
    v_rgb = torch.as_tensor(v_rgb, dtype=torch.float32).to(dev).contiguous()
    if tuple(v_rgb.shape) != (V, 3):
        raise ValueError("%s: v_rgb is %s, the mesh has %d vertices: expected [%d, 3]" % (who, tuple(v_rgb.shape), V, V))
    weights = torch.as_tensor(weights, dtype=torch.float32).to(dev).contiguous()
    if tuple(weights.shape) != (B,):
        raise ValueError("%s: weights is %s, expected [%d]" % (who, tuple(weights.shape), B))
    if isinstance(render_size, (tuple, list)):
        raise ValueError("%s: render_size is one number (the dilation radius is render_size // 512)" % who)
    visible = r.get_visible_vertices(c2ws, perspective=perspective, method="raster", intrinsics=intrinsics, render_size=int(render_size), erode_neighbor=0)
    ret = r.simple_rendering(c2ws, intrinsics, int(render_size), perspective=perspective, render_cos_ray_normal=True, render_camera_normal=not perspective)
    wmap = ops.view_weight_maps(ret["cos_ray_normal"], None if perspective else ret["camera_normal"], r=ops.weight_map_radius(render_size))
    xform = (c2ws if reference_transform else camera.c2w_to_w2c(c2ws)).to(dev).contiguous()
    proj = camera.intr_to_proj(intrinsics, perspective=perspective).to(dev).contiguous()
    return ops.vertex_project(m.vertices, visible.to(torch.uint8).contiguous(), xform, proj, images, wmap, v_rgb, weights, use_alpha=use_alpha, epilogue=epilogue)


def project_vertex_color(mesh, c2ws, intrinsics, images, v_rgb, weights, use_alpha=True, render_size=512, visualize=False, perspective=True,
                         reference_transform=False):
    """c2ws [B,4,4], intrinsics [B,3,3] (or [3,3]), images [B,4,H,W] rgba, v_rgb [V,3], weights [B] -> (v_rgb_acc [V,3], v_weight_acc [V,1]).
    The vertices a view sees (get_visible_vertices, the raster method at render_size, no erosion: a default-constructed reference renderer) that project
    strictly inside the view take its colour -- sampled bilinearly with reflection padding, blended over v_rgb with the image's alpha unless
    use_alpha=False -- with the weight weights[b] * cos^4 * (1 - edge alpha), both sampled from the view's weight maps (ops.view_weight_maps on
    simple_rendering's cos_ray_normal; orthographic: camera_normal.z); v_rgb_acc = sum of weight * colour, v_weight_acc = sum of weight, views in index
    order.  reference_transform: see the module docstring."""
    _refuse_visualize("project_vertex_color", visualize)
    return _project("project_vertex_color", mesh, c2ws, intrinsics, images, v_rgb, weights, use_alpha, render_size, perspective, reference_transform, None)


def remapping_vertex_color(mesh, c2ws, intrinsics, images, v_rgb=None, weights=None, use_alpha=True, overlay_confidence=0.2, use_blending=True,
                           blending_type="soft", blending_confidence=0.2, use_inpainting=True, inpainting_confidence=0.2, render_size=512, visualize=False,
                           perspective=True, reference_transform=False, return_stages=False):
    """project_vertex_color, then (:326-349): overlay -- the accumulated colour divided by the accumulated weight where that exceeds overlay_confidence;
    blending against v_rgb where the weight is at most blending_confidence ('soft': (v_rgb * (conf - w) + acc) / conf, 'hard': v_rgb); inpainting of
    the vertices whose weight is at most inpainting_confidence (inpainting_vertex_color).  v_rgb=None: zeros and no blending.  weights=None: the
    reference's table for 8 / 6 / 4 / 2 views, ones otherwise.  Returns v_rgb [V,3]; with return_stages=True a dict of every stage as well
    (v_rgb_acc, v_weight_acc, blended, inpaint_mask, v_rgb, inpaint_steps).  A weights of the wrong length and an unknown blending_type raise
    ValueError (the reference's two assertions)."""
    _refuse_visualize("remapping_vertex_color", visualize)
    batch_size = torch.as_tensor(c2ws).shape[0]
    if weights is not None and len(weights) != batch_size:
        raise ValueError("size mismatch: length of weights should be %d but %d" % (batch_size, len(weights)))
    if blending_type not in ("soft", "hard"):
        raise ValueError("value error: %s is not supported" % (blending_type,))
    r = _renderer(mesh)
    if v_rgb is None:
        v_rgb = torch.zeros_like(r.pbr_mesh.vertices)
        use_blending = False
    if weights is None:
        weights = default_weights(batch_size)
    weights = torch.as_tensor(np.asarray(weights, dtype=np.float32))
    epilogue = dict(overlay_confidence=overlay_confidence, blending=blending_type if use_blending else None, blending_confidence=blending_confidence,
                    inpainting_confidence=inpainting_confidence)
    acc, wacc, blended, mask = _project("remapping_vertex_color", r, c2ws, intrinsics, images, v_rgb, weights, use_alpha, render_size, perspective,
                                        reference_transform, epilogue)
    out, steps = blended, 0
    if use_inpainting:
        rowptr, col = _adjacency(r.pbr_mesh)
        out, steps = ops.vertex_inpaint(rowptr, col, blended, torch.nonzero(mask)[:, 0], max_iters=1000)
    if return_stages:
        return out, dict(v_rgb_acc=acc, v_weight_acc=wacc, blended=blended, inpaint_mask=mask, v_rgb=out, inpaint_steps=steps)
    return out


def inpainting_vertex_color(mesh, v_rgb, v_idx_inpainting, max_iters=1000, return_steps=False):
    """v_rgb [V,3], v_idx_inpainting [n]: the vertices to fill.  Each step gives every vertex of the list the mean of its valid neighbours and makes it
    valid if it has one; the list never shrinks (filled vertices are averaged again); the loop ends when a step added no vertex (that step is kept) or
    after max_iters.  A vertex whose component holds no valid vertex keeps its colour.  Returns a new tensor (the reference writes into v_rgb);
    return_steps=True: (v_rgb, number of steps)."""
    r = _renderer(mesh)
    m = r.pbr_mesh
    v_rgb = torch.as_tensor(v_rgb, dtype=torch.float32).to(r.device).contiguous()
    V = m.vertices.shape[0]
    if tuple(v_rgb.shape) != (V, 3):
        raise ValueError("inpainting_vertex_color: v_rgb is %s, the mesh has %d vertices: expected [%d, 3]" % (tuple(v_rgb.shape), V, V))
    idx = torch.as_tensor(v_idx_inpainting).to(r.device).reshape(-1)
    if idx.numel() and not bool(((idx >= 0) & (idx < V)).all()):      # one read-back
        raise ValueError("inpainting_vertex_color: v_idx_inpainting reaches outside the %d vertices" % V)
    rowptr, col = _adjacency(m)
    out, steps = ops.vertex_inpaint(rowptr, col, v_rgb, idx, max_iters=max_iters)
    return (out, steps) if return_steps else out


def initial_map_Kd_with_v_rgb(mesh, v_rgb, texture_size=1024, use_pymeshlab=False, use_cv_outpainting=False, visualize=False, perspective=True):
    """The vertex colours as an atlas [H,W,4]: v_rgb interpolated into the UV raster (simple_inverse_rendering(render_v_attr=True)), the texels outside
    the charts filled by pull_push from the mask alpha > 0.6, alpha = compute_uv_mask.  Existing ops only.  perspective is accepted and unused: the
    atlas raster has no camera."""
    _refuse_visualize("initial_map_Kd_with_v_rgb", visualize)
    if use_pymeshlab:
        raise NotImplementedError("initial_map_Kd_with_v_rgb(use_pymeshlab=True) is not built")
    if use_cv_outpainting:
        raise NotImplementedError("initial_map_Kd_with_v_rgb(use_cv_outpainting=True) is not built: the outpainting is pull_push")
    r = _renderer(mesh)
    alpha = r.compute_uv_mask(texture_size=texture_size).to(torch.float32)
    rgb = r.simple_inverse_rendering(None, texture_size, render_v_attr=True, v_attr=v_rgb, enable_antialis=False)["v_attr"][0]
    filled = ops.pull_push(rgb[..., :3].contiguous(), (alpha[..., 0] > 0.6).to(torch.uint8).contiguous())
    return torch.cat([filled, alpha], dim=-1)
