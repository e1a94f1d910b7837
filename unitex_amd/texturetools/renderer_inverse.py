"""NVDiffRendererInverse -- MI355X-native drop-in for the reference's multi-view -> UV back-projection
(TextureTools/texturetools/render/nvdiffrast/renderer_inverse.py).

Kept call surface (as the reference orchestrator uses it, /root/reference/pipeline.py:330-359):
    inv = NVDiffRendererInverse(device='cuda')
    inv.update_from_file(mesh_path)
    textured_mesh, mask_2d_visiable, mask_2d, color_2d = inv.infer(mesh_path, c2ws=..., intrinsics=...,
        image_attrs=[6,H,W,3], perspective=False, H=, W=, H2D=, W2D=, method='reproject', ...)
    perspective=True (the reference's default) casts each ray from the camera centre c2w[:3, 3] to the surface point
    (renderer_inverse.py:187-190, 279-281); perspective=False, the pipeline's cameras, casts parallel rays along -c2w[:3, 2].
    inv.clear();  inv.register_query_field(fn)

What runs where: every per-texel stage is a HIP kernel behind the C ABI (ops.py): clip transform,
UV-space raster, fused gather + LBVH visibility, hole filling, priority composite, seam mask, exact 3-D
NN fill, seam lens blur, pull-push, uint8 conversion.  No [6,2048,2048,3] intermediates other than the
per-view colour layers that the composite (and, multi-GPU, the all-gather) consumes.

Nine channels (the PBR stack: albedo 0:3, metallic-roughness 3:6, bump 6:9; renderer_inverse.py:716-721) with method='reproject' take a path of
their own, because nothing in visibility, winner, seam or the nearest-neighbour search reads colour: visibility-only back-projection, winner from
visibility, seam, then ONE gather of the nine channels from each texel's winning view, and C-channel fill / blur / pull-push.  No per-view colour
layer exists on that path, and a view shard exchanges the u8 visibility layers only.

Multi-GPU: views are sharded over ranks (`view_shard=(rank, world)`); each rank fills its
views' colour/visibility layers, ONE all_gather (RCCL over xGMI, or gloo in the CPU tests) assembles the
layers, and the composite + post-processing run replicated on every rank.
"""
import contextlib
import time
import os
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import camera, meshes, ops

PRIORITY = [0, 3, 4, 1, 2, 5]  # frtbld -> f, b, l, r, t, d  (reference renderer_inverse.py:44)


_UNSET = object()      # 'the keyword was not passed' (simple_inverse_rendering takes intrinsics only with render_uv)


def _check_seam_sizes(k_boundary, k_boundary_blur):
    """the seam windows of bake_mv_to_uv_reproject_blur: 2 (k // 2) + 1 wide, so any k >= 0; radii above ops.SEAM_RADIUS_MAX are not built"""
    for name, k in (("reproject_kernel_size_boundary", k_boundary), ("reproject_kernel_size_boundary_blur", k_boundary_blur)):
        if int(k) != k or k < 0:
            raise ValueError("%s should be a non-negative integer. Got %r" % (name, k))
        if k // 2 > ops.SEAM_RADIUS_MAX:
            raise NotImplementedError("%s=%r: the seam mask is built up to a radius of %d (%s <= %d)" % (name, k, ops.SEAM_RADIUS_MAX, name,
                                                                                                          2 * ops.SEAM_RADIUS_MAX + 1))


def _check_gaussian_ksize(k):
    """torchvision's gaussian_blur checks (ValueError for an even or negative size), then this build's cap"""
    if int(k) != k or k % 2 == 0 or k < 0:
        raise ValueError("kernel_size should have odd and positive integers. Got %r" % ([k, k],))
    if k > ops.GAUSS_KSIZE_MAX:
        raise NotImplementedError("reproject_kernel_size_blur=%r: the Gaussian seam blur is built up to a kernel size of %d" % (k, ops.GAUSS_KSIZE_MAX))


def _refuse_unbuilt(who, kwargs, known):
    """the reference's flags that simple_inverse_rendering / simple_rendering do not build: one of `known` is refused when set, any other keyword is
    a TypeError"""
    for k_, v_ in kwargs.items():
        if k_ not in known:
            raise TypeError("%s() got an unexpected keyword argument %r" % (who, k_))
        if v_:
            raise NotImplementedError("%s(%s=%r) is not built" % (who, k_, v_))


def _check_grid_interpolate_mode(who, mode):
    if mode not in ops.SCREEN_FILTERS:
        raise ValueError("%s(grid_interpolate_mode=%r): one of %s" % (who, mode, ", ".join(ops.SCREEN_FILTERS)))


def _reads_vertex_normals(want):
    """does a buffer of `want` read the vertex normals?  (they are built lazily, on the host; the atlas and the screen name these buffers alike)"""
    return any(k in ("world_normal",) + ops.SCREEN_GBUFFERS_NRM_CAM for k in want)


class DeviceMesh:
    """PBRMesh of the reference (mesh/structure_v2.py:25-77) reduced to what the inverse renderer reads:
    vertices, faces, per-face normals, UVs mapped to [-1, 1], and the lazily built LBVH ('optix')."""

    def __init__(self, verts, faces, uvs, device):
        self.device = torch.device(device)
        self.vertices = torch.as_tensor(verts, dtype=torch.float32).to(self.device).contiguous()
        self.faces = torch.as_tensor(faces, dtype=torch.int32).to(self.device).contiguous()
        self.uvs01 = np.asarray(uvs, dtype=np.float32)
        self.uvs_2d = (torch.as_tensor(uvs, dtype=torch.float32) * 2.0 - 1.0).to(self.device).contiguous()  # structure_v2.py:287
        self.normals = ops.face_normals(self.vertices, self.faces)      # HIP, bit-exact vs the oracle's op order
        self._bvh = None
        self._vertex_normals = None
        self._edge_opposites = None

    @property
    def vertex_normals(self):
        """area-weighted vertex normals (mesh/structure_v2.py:64-71: face cross products scattered to the corners, normalised)."""
        if self._vertex_normals is None:
            from .video import _vertex_normals
            self._vertex_normals = _vertex_normals(self.vertices.cpu(), self.faces.cpu(), weighting="area").to(self.device)
        return self._vertex_normals

    @property
    def edge_opposites(self):
        """[F,3] int32 on the device: the vertex across each edge, -1 on a border (meshes.edge_opposites; built on the host once per mesh)"""
        if getattr(self, "_edge_opposites", None) is None:
            self._edge_opposites = torch.from_numpy(meshes.edge_opposites(self.faces.cpu().numpy())).to(self.device).contiguous()
        return self._edge_opposites

    def set_vertex_normals(self, normals):
        """per-vertex normals [V,3] of the caller's own (e.g. the file's, or analytic ones) in place of the area-weighted ones; they need not be unit"""
        n = torch.as_tensor(normals, dtype=torch.float32).to(self.device).contiguous()
        assert tuple(n.shape) == tuple(self.vertices.shape), "one normal per vertex"
        self._vertex_normals = n
        return self

    @property
    def optix(self):
        if self._bvh is None:
            self._bvh = ops.BVH(self.vertices, self.faces)
        return self._bvh


def load_device_mesh(path, device):
    verts, faces, uvs, _ = meshes.load_mesh(path)        # .obj / .glb / .gltf / .ply / .stl / .off
    if uvs is None:
        raise ValueError("mesh %s has no UVs: run it through meshes.prepare_blank_mesh (pipeline.preprocess_blank_mesh) first" % path)
    return DeviceMesh(verts, faces, uvs, device)


def _check_channels(shape):
    """the reference bakes rgb or the 9-channel PBR stack with either method and refuses anything else (renderer_inverse.py:709-724)"""
    if shape[-1] not in (3, 9):
        raise NotImplementedError("shape %s is not supported" % (torch.Size(shape),))


class TexturedMesh:
    """what infer() returns in place of a trimesh.Trimesh: exposes .export(path) for .glb / .obj.
    .texture is the albedo (uint8 [H,W,3], top row first, i.e. already flipped as link_rgb_to_mesh / link_pbr_to_mesh flip it).  A 9-channel bake also
    carries .metallic_roughness and .bump, converted and flipped the same way (link_pbr_to_mesh, io/link_pbr_to_mesh.py:34-60); both are None for an
    rgb bake.  link_*_to_mesh's merge_vertices / fix_normals are trimesh calls on its own mesh object and are not reproduced: vertices, faces and UVs
    are the blank mesh's, unchanged.
    export('.glb') writes the three images as baseColorTexture / metallicRoughnessTexture / normalTexture with no factors (the reference passes None for
    all three, so glTF's defaults apply).  export('.obj') writes <base>.png, <base>_metallic_roughness.png and <base>_bump.png and names them in the
    .mtl as map_Kd / map_Pm / map_Bump; trimesh's own .mtl keys for a PBRMaterial are third-party code that is not available here, so the two extra
    keys are this build's choice."""

    def __init__(self, verts, faces, uvs01, texture_u8_top_down, metallic_roughness=None, bump=None):
        self.vertices, self.faces, self.uv, self.texture = verts, faces, uvs01, texture_u8_top_down
        self.metallic_roughness, self.bump = metallic_roughness, bump

    def export(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        pbr = self.metallic_roughness is not None
        if path.lower().endswith(".glb"):
            if pbr:
                meshes.save_glb(path, self.vertices, self.faces, self.uv, self.texture, metallic_roughness_u8=self.metallic_roughness, bump_u8=self.bump)
            else:
                meshes.save_glb(path, self.vertices, self.faces, self.uv, self.texture)
        else:
            from PIL import Image
            base = os.path.splitext(path)[0]
            level = int(os.environ.get("UTX_PNG_LEVEL", "1"))
            Image.fromarray(self.texture).save(base + ".png", compress_level=level)
            mtl = "newmtl material_0\nmap_Kd %s\n" % os.path.basename(base + ".png")
            if pbr:
                for key, suffix, img in (("map_Pm", "_metallic_roughness", self.metallic_roughness), ("map_Bump", "_bump", self.bump)):
                    Image.fromarray(img).save(base + suffix + ".png", compress_level=level)
                    mtl += "%s %s\n" % (key, os.path.basename(base + suffix + ".png"))
            with open(base + ".mtl", "w") as f:
                f.write(mtl)
            meshes.save_obj(path, self.vertices, self.faces, self.uv, mtl=os.path.basename(base + ".mtl"))
        return path


class NVDiffRendererInverse:
    def __init__(self, device="cuda", pbr_mesh: Optional[DeviceMesh] = None, view_shard: Tuple[int, int] = (0, 1),
                 process_group=None):
        self.device = torch.device(device if device != "cuda" else "cuda:%d" % torch.cuda.current_device())
        self.pbr_mesh = pbr_mesh
        self.index = list(PRIORITY)
        self.query_field_function = None
        self.view_shard = view_shard
        self.process_group = process_group
        self.last = {}
        self.stage_events = None   # set to [] to collect (stage, start_event, end_event) per infer() stage

    @contextlib.contextmanager
    def _stage(self, name):
        """optional HIP-event bracket per stage (bench.py / tools/bench_backproject.py); no sync, no cost when off."""
        if self.stage_events is None:
            yield
            return
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        yield
        b.record()
        self.stage_events.append((name, a, b))

    # ---- reference surface
    def clear(self):
        self.pbr_mesh = None
        self.query_field_function = None

    def update_from_file(self, pbr_mesh_path=None):
        assert pbr_mesh_path is not None
        self.pbr_mesh = load_device_mesh(pbr_mesh_path, self.device)
        return self

    def update_from_arrays(self, verts, faces, uvs):
        self.pbr_mesh = DeviceMesh(verts, faces, uvs, self.device)
        return self

    def register_query_field(self, query_field: Optional[Callable] = None):
        self.query_field_function = query_field
        return self

    # ---- stages
    def _mvp(self, c2ws, intrinsics, perspective):
        c2ws = torch.as_tensor(c2ws, dtype=torch.float32).cpu()
        intr = torch.as_tensor(intrinsics, dtype=torch.float32).cpu()
        mvp = torch.matmul(camera.intr_to_proj(intr, perspective=perspective), camera.c2w_to_w2c(c2ws))
        return mvp.to(self.device).contiguous(), c2ws

    def _view_raster(self, c2ws, intrinsics, render_size, perspective):
        """the cameras' clip transform and one rasterisation per view (mv_to_pcd and simple_rendering share it):
        (mvp [n,4,4], c2ws on the host, clip [n,V,4], ndc [n,V,2], rast [n,H,W,4])"""
        H, W = (render_size, render_size) if isinstance(render_size, int) else render_size
        m = self.pbr_mesh
        mvp, c2ws_cpu = self._mvp(c2ws, intrinsics, perspective)
        clip, ndc = ops.transform_points(m.vertices, mvp)
        n = mvp.shape[0]
        rast = torch.empty(n, H, W, 4, dtype=torch.float32, device=self.device)
        for v in range(n):
            rast[v] = ops.rasterize(clip[v].contiguous(), m.faces, H, W)
        return mvp, c2ws_cpu, clip, ndc, rast

    def mv_to_pcd(self, c2ws, intrinsics, render_size, perspective=True, grad_norm_threhold=0.20, ray_normal_angle_threhold=115.0,
                  filt_gradient_points=False, want_points=False):
        """view-space pass of the reference's mv_to_pcd (renderer_inverse.py:159-241), dense instead of compacted:
          alpha [n,H,W] f32 = mask_visiable as float: plain coverage, or with filt_gradient_points=True coverage AND
          back-facing-ray test AND the (row-wise, 31 wide) eroded gradient test (:189-209);
          want_points: also pos [n,H,W,3] (interpolated vertex positions = the point cloud of :224-232) and the raster."""
        m = self.pbr_mesh
        mvp, c2ws_cpu, clip, ndc, rast = self._view_raster(c2ws, intrinsics, render_size, perspective)
        n, H, W = rast.shape[:3]
        out = {"clip": clip, "ndc": ndc}
        attrs = None
        if filt_gradient_points or want_points:
            va = torch.cat([m.vertices, m.vertex_normals], dim=-1).contiguous()
            attrs = ops.interpolate(va, rast.view(n * H, W, 4), m.faces).view(n, H, W, 6)
        if filt_gradient_points:
            if perspective:     # rays from the camera centre through each pixel's surface point (:187-189)
                eyes = c2ws_cpu[:, :3, 3].contiguous().to(self.device)
                vis, alpha = ops.view_visibility(attrs, rast, m.normals, None, grad_thr=grad_norm_threhold, angle_deg=ray_normal_angle_threhold,
                                                 eyes=eyes)
            else:
                dirs = torch.nn.functional.normalize(-c2ws_cpu[:, :3, 2], dim=-1).contiguous().to(self.device)
                vis, alpha = ops.view_visibility(attrs, rast, m.normals, dirs, grad_thr=grad_norm_threhold, angle_deg=ray_normal_angle_threhold)
        else:
            alpha = (rast[..., 3] > 0).float()
            vis = (rast[..., 3] > 0).to(torch.uint8)
        out["alpha"], out["mask_visiable"] = alpha, vis
        if want_points:
            out["pos"] = attrs[..., :3].contiguous()
            out["rast"] = rast
        return out

    def query_field(self, vertices_visiable, colors_visiable, vertices_invisiable):
        """the LTM hook (renderer_inverse.py:143-157): colours for unseen points from the seen ones."""
        if self.query_field_function is None:
            raise NotImplementedError("using register_query_field before query")
        return self.query_field_function(vertices_visiable, colors_visiable, vertices_invisiable)

    def _fill_unseen(self, atlas, seen_u8, covered, pos, inpainting, k=1):
        """colours for covered-but-unseen texels, in place on atlas [H2D,W2D,C]: the k nearest seen texels in 3-D (mean),
        or the registered query field (renderer_inverse.py:420-426 / :606-615)."""
        unseen = covered & (seen_u8 == 0)
        if inpainting:
            seen_b = seen_u8.bool()
            col = self.query_field(pos[seen_b], atlas[seen_b], pos[unseen])      # compaction only at this (user) boundary
            atlas[unseen] = torch.as_tensor(col, dtype=torch.float32, device=atlas.device)
        else:
            ops.knn_gather(pos, pos, k, src_attr=atlas, src_mask=seen_u8, dst_mask=unseen.to(torch.uint8), out=atlas.view(-1, atlas.shape[-1]))
        return unseen

    def _bake_kdtree(self, mv, images, vis, rast2d, pos2d, method, k_all, k_vis, k_inv, inpainting):
        """bake_mv_to_uv_kdtree (renderer_inverse.py:367-433) on dense layers.
        mv: view pass (pos [n,H,W,3], mask_visiable [n,H,W]); images [n,H,W,C]; vis [n,H2D,W2D] u8; pos2d [H2D,W2D,3]."""
        n, Hh, Ww, C = images.shape
        H2D, W2D = rast2d.shape[:2]
        covered = rast2d[..., 3] > 0
        cov_u8 = covered.to(torch.uint8)
        atlas = torch.zeros(H2D, W2D, C, dtype=torch.float32, device=self.device)
        if method in ("mean", "mvpaint"):
            if method == "mean" and inpainting:
                b = mv["mask_visiable"].bool()
                col = self.query_field(mv["pos"][b], images[b], pos2d[covered])
                atlas[covered] = torch.as_tensor(col, dtype=torch.float32, device=self.device)
            else:
                kw = {}
                if method == "mvpaint":   # both point clouds carry FACE normals (renderer_inverse.py:226-233, 350)
                    tid = (mv["rast"][..., 3].long() - 1).clamp_(min=0)
                    tid2 = (rast2d[..., 3].long() - 1).clamp_(min=0)
                    kw = dict(mode="mvpaint", src_nrm=self.pbr_mesh.normals[tid.view(-1)], dst_nrm=self.pbr_mesh.normals[tid2.view(-1)])
                ops.knn_gather(mv["pos"], pos2d, k_all, src_attr=images, src_mask=mv["mask_visiable"], dst_mask=cov_u8,
                               out=atlas.view(-1, C), **kw)
        elif method == "order_mean":
            current = torch.zeros(H2D, W2D, dtype=torch.bool, device=self.device)
            for i in self.index:
                extra = (~current) & vis[i].bool()
                ops.knn_gather(mv["pos"][i], pos2d, k_vis, src_attr=images[i], src_mask=mv["mask_visiable"][i],
                               dst_mask=extra.to(torch.uint8), out=atlas.view(-1, C))
                current |= extra
            self._fill_unseen(atlas, (current & covered).to(torch.uint8), covered, pos2d, inpainting, k=k_inv)
        else:
            raise NotImplementedError("method %s is not supported" % method)
        return atlas

    def _uv_raster(self, H2D, W2D):
        """UV-space raster [H2D,W2D,4]: uv in [-1,1] used directly as clip xy, z = 0, w = 1 (renderer_inverse.py:268-274, renderer_base.py:377-384)"""
        m = self.pbr_mesh
        uvclip = torch.cat([m.uvs_2d, torch.zeros_like(m.uvs_2d[:, :1]), torch.ones_like(m.uvs_2d[:, :1])], dim=-1).contiguous()
        with self._stage("uv_raster"):
            return ops.rasterize(uvclip, m.faces, H2D, W2D)

    # flag of simple_inverse_rendering -> key of the returned dict, camera-independent first
    _UV_FLAGS = ("world_normal", "world_position", "camera_normal", "camera_position", "distance", "z_depth", "ray_direction", "cos_ray_normal")
    _UV_FLAGS_UNBUILT = ("render_voxel_attr", "render_all_point_cloud", "render_visible_point_cloud")

    def simple_inverse_rendering(self, c2ws=None, texture_size=2048, render_world_normal=False, render_world_position=False,
                                 render_camera_normal=False, render_camera_position=False, render_distance=False, render_z_depth=False,
                                 render_ray_direction=False, render_cos_ray_normal=False, enable_antialis=True, render_v_attr=False, v_attr=None,
                                 background=None, intrinsics=_UNSET, perspective=True, map_attr=None, render_uv=False, render_map_attr=False,
                                 grid_interpolate_mode="bilinear", visible_faces="rays", **kwargs):
        """NVDiffRendererBase.simple_inverse_rendering (render/nvdiffrast/renderer_base.py:352-489) on the mesh of update_from_file: the geometry
        buffers rendered into the UV atlas instead of onto a screen, all of them in one kernel launch (ops.uv_gbuffer).  Returns the reference's
        dict: 'mask' bool [1,H,W,1], 'alpha' float32 [1,H,W,1] and, per flag, 'world_normal' / 'world_position' [1,H,W,3] and, per camera of
        c2ws [B,4,4], 'camera_normal' / 'camera_position' / 'ray_direction' [B,H,W,3], 'distance' / 'z_depth' / 'cos_ray_normal' [B,H,W,1].
        texture_size: int or (H, W).  Row 0 is v = 0 (the raster's orientation; TexturedMesh.texture is the flipped one).  Only c2ws enters: the
        function never projects, so it takes no intrinsics.  Vertex normals are pbr_mesh.vertex_normals.
        enable_antialis is accepted and has no effect: alpha is the coverage mask (dr.antialias is not wired here: ops.antialias serves simple_rendering(antialias=True) only).
        render_v_attr (:491-502) adds 'v_attr' [1,H,W,Ca]: the per-vertex attribute v_attr [V,Ca] interpolated into the atlas by the screen kernel
        (ops.screen_gbuffer on the atlas raster as a batch of one), then the background rule of simple_rendering: None leaves the interpolated value
        (0 outside the charts), a number or a tensor that broadcasts to [1,H,W,Ca] fills the uncovered texels.
        A camera-dependent flag without c2ws raises ValueError, and so does a v_attr that is not [V,Ca]; render_v_attr with no v_attr at all is
        refused like an unbuilt flag (NotImplementedError: the mesh has no attribute of its own to render); render_voxel_attr,
        render_all_point_cloud and render_visible_point_cloud are not built and raise NotImplementedError when set; any other keyword is a TypeError.
        render_uv (:504-536) projects the cameras c2ws [B,4,4] / intrinsics [B,3,3] into the atlas: 'uv_alpha' [B,H,W,1], 1 on the texels whose
        face the view sees, and 'uv' [B,H,W,2], the view's NDC of the texel's surface point (-1 elsewhere).  The faces a view sees come from
        get_visible_faces: visible_faces='rays' (the reference's Mesh.get_visible_faces) or 'raster' (its commented-out twin, :512), which
        rasterises at the size of map_attr and therefore needs one.  perspective replaces the reference's enable_perspective() /
        enable_orthogonal() state, as in simple_rendering; intrinsics is taken only with render_uv -- nothing else projects -- and is a
        TypeError without it.  render_map_attr (:538-559) adds 'map_attr' [B,H,W,C]: map_attr [Hm,Wm,C], [1,Hm,Wm,C] or [B,Hm,Wm,C] (one image
        per view) sampled at 'uv' with grid_interpolate_mode ('bilinear' | 'nearest' | 'nvdiffrast', as simple_rendering); the views are
        rasterised once more at the map's size and 'uv_alpha' drops to 0 where the view's coverage, looked up at uv, is missing; background
        None puts the map's texel [0, 0] there, a number or a tensor that broadcasts to [B,H,W,C] fills every texel with uv_alpha = 0.  One
        kernel launch (ops.uv_project) for all views.  render_uv together with the camera-dependent geometry flags equals the separate calls
        (the reference cannot make that call: :446 rebinds batch_size to a torch.Size, which :514 then hands to Tensor.tile).
        render_uv without cameras and render_map_attr without render_uv raise NotImplementedError; c2ws without intrinsics, render_map_attr
        without map_attr, a map of the wrong rank or of a batch that is neither 1 nor B, an unknown visible_faces or grid_interpolate_mode
        raise ValueError."""
        _refuse_unbuilt("simple_inverse_rendering", kwargs, self._UV_FLAGS_UNBUILT)
        if intrinsics is not _UNSET and not render_uv:
            raise TypeError("simple_inverse_rendering() takes intrinsics only with render_uv=True: no other buffer projects")
        if render_map_attr and not render_uv:
            raise NotImplementedError("simple_inverse_rendering(render_map_attr=True) without render_uv is not built: the map is sampled at 'uv'")
        if render_uv:
            if c2ws is None:
                raise NotImplementedError("simple_inverse_rendering(render_uv=True) without cameras is not built: pass c2ws and intrinsics")
            if intrinsics is _UNSET or intrinsics is None:
                raise ValueError("simple_inverse_rendering(render_uv=True) projects the cameras: intrinsics is required")
            _check_grid_interpolate_mode("simple_inverse_rendering", grid_interpolate_mode)
            if visible_faces not in ("rays", "raster"):
                raise ValueError("simple_inverse_rendering(visible_faces=%r): 'rays' or 'raster'" % (visible_faces,))
            n_views = torch.as_tensor(c2ws).shape[0]
            if render_map_attr:
                if map_attr is None:
                    raise ValueError("simple_inverse_rendering(render_map_attr=True) needs map_attr")
                map_attr = torch.as_tensor(map_attr, dtype=torch.float32)
                if map_attr.dim() == 3:
                    map_attr = map_attr[None]
                if map_attr.dim() != 4 or min(map_attr.shape) < 1:
                    raise ValueError("simple_inverse_rendering: map_attr is %s, expected [Hm, Wm, C], [1, Hm, Wm, C] or [B, Hm, Wm, C]" % (tuple(map_attr.shape),))
                if map_attr.shape[0] not in (1, n_views):
                    raise ValueError("simple_inverse_rendering: map_attr holds %d images, the call has %d cameras: 1 or one per camera" % (map_attr.shape[0], n_views))
            elif visible_faces == "raster":
                raise ValueError("simple_inverse_rendering(visible_faces='raster') rasterises at the size of map_attr: set render_map_attr and pass one")
        if render_v_attr and v_attr is None:      # the mesh carries no per-vertex attribute of its own that could stand in
            raise NotImplementedError("simple_inverse_rendering(render_v_attr=True) without v_attr is not built: pass v_attr [V, Ca]")
        flags = dict(world_normal=render_world_normal, world_position=render_world_position, camera_normal=render_camera_normal,
                     camera_position=render_camera_position, distance=render_distance, z_depth=render_z_depth,
                     ray_direction=render_ray_direction, cos_ray_normal=render_cos_ray_normal)
        want = [k for k in self._UV_FLAGS if flags[k]]
        per_view = [k for k in want if ops.UV_GBUFFERS[k][2]]
        if per_view and c2ws is None:
            raise ValueError("simple_inverse_rendering(render_%s=True) depends on the cameras: c2ws is required" % per_view[0])
        H2D, W2D = (texture_size, texture_size) if isinstance(texture_size, int) else texture_size
        m = self.pbr_mesh
        assert m is not None, "update_from_file first"
        if render_v_attr:
            v_attr = self._vertex_attr(v_attr, "simple_inverse_rendering")
        rast2d = self._uv_raster(int(H2D), int(W2D))
        with self._stage("uv_gbuffer"):
            out = ops.uv_gbuffer(rast2d, m.faces, m.vertices, m.vertex_normals if _reads_vertex_normals(want) else None, c2ws=c2ws,
                                 want=["mask", "alpha"] + want)
            if render_v_attr:
                out["v_attr"] = ops.screen_gbuffer(rast2d[None], m.faces, m.vertices, v_attr=v_attr, want=("v_attr",), background=background)["v_attr"]
        if render_uv:
            rast_map = None
            if render_map_attr:
                map_attr = map_attr.to(self.device).contiguous()
                with self._stage("view_raster"):
                    _, _, _, ndc, rast_map = self._view_raster(c2ws, intrinsics, tuple(map_attr.shape[1:3]), perspective)
            else:
                ndc = ops.transform_points(m.vertices, self._mvp(c2ws, intrinsics, perspective)[0])[1]
            with self._stage("visible_faces"):
                face_mask = self._visible_faces(c2ws, perspective, visible_faces, rast_map, 0)
            with self._stage("uv_project"):
                out.update(ops.uv_project(rast2d, m.faces, face_mask, ndc, map_attr if render_map_attr else None, rast_map,
                                          filter=grid_interpolate_mode, background=background))
        out["mask"] = out["mask"].bool()[None, ..., None]
        out["alpha"] = out["alpha"][None]
        return out

    def _visible_faces(self, c2ws, perspective, method, rast, erode_neighbor):
        """face mask uint8 [B,F] on the device: method 'rays' on the mesh's cached tree, 'raster' from the views' rasters rast [B,H,W,4]"""
        m = self.pbr_mesh
        if method == "rays":
            mask = ops.visible_faces_rays(m.optix, torch.as_tensor(c2ws, dtype=torch.float32).to(self.device).contiguous(), perspective=perspective)
        else:
            mask = ops.visible_faces_raster(rast, m.faces.shape[0])
        if erode_neighbor > 0:
            mask = ops.erode_faces(mask, m.faces, m.vertices.shape[0], erode_neighbor)
        return mask

    def _visible_faces_checked(self, who, c2ws, perspective, method, intrinsics, render_size, erode_neighbor):
        if method not in ("rays", "raster"):
            raise ValueError("%s(method=%r): 'rays' or 'raster'" % (who, method))
        if method == "raster" and (intrinsics is None or render_size is None):
            raise ValueError("%s(method='raster') rasterises the views: intrinsics and render_size are required" % who)
        if int(erode_neighbor) < 0:
            raise ValueError("%s(erode_neighbor=%r): a number of rounds >= 0" % (who, erode_neighbor))
        c2ws = torch.as_tensor(c2ws, dtype=torch.float32)
        if c2ws.dim() != 3 or tuple(c2ws.shape[1:]) != (4, 4) or c2ws.shape[0] < 1:
            raise ValueError("%s: c2ws is %s, expected [B >= 1, 4, 4]" % (who, tuple(c2ws.shape)))
        assert self.pbr_mesh is not None, "update_from_file first"
        rast = self._view_raster(c2ws, intrinsics, render_size, perspective)[4] if method == "raster" else None
        return self._visible_faces(c2ws, perspective, method, rast, int(erode_neighbor))

    def get_visible_faces(self, c2ws, perspective=True, method="rays", intrinsics=None, render_size=None, erode_neighbor=0):
        """The faces each camera of c2ws [B,4,4] sees, bool [B,F], on the mesh of update_from_file / update_from_arrays.
        method='rays' is Mesh.get_visible_faces of the reference (mesh/structure.py:801-844): one ray per face, aimed at its centroid (perspective:
        from the camera centre; orthographic: along the view direction), marks the face it hits FIRST -- closest hit on the mesh's cached tree,
        no backface culling -- so a face is visible iff some ray of the view lands on it.  method='raster' is NVDiffRendererBase.get_visible_faces
        (render/nvdiffrast/renderer_base.py:65-85): the faces whose id appears in the view rasterised at render_size with intrinsics [B,3,3]
        (both required; ValueError without them).  erode_neighbor > 0 applies erode_face that many times (the reference's self.erode_neighbor,
        which only its raster twin reads; here either method takes it)."""
        return self._visible_faces_checked("get_visible_faces", c2ws, perspective, method, intrinsics, render_size, erode_neighbor).bool()

    def get_visible_vertices(self, c2ws, perspective=True, method="rays", intrinsics=None, render_size=None, erode_neighbor=0):
        """The vertices each camera sees, bool [B,V]: those of the faces of get_visible_faces (same arguments; structure.py:846-857,
        renderer_base.py:87-99)."""
        mask = self._visible_faces_checked("get_visible_vertices", c2ws, perspective, method, intrinsics, render_size, erode_neighbor)
        return ops.visible_vertices(mask, self.pbr_mesh.faces, self.pbr_mesh.vertices.shape[0]).bool()

    def _vertex_attr(self, v_attr, who):
        """v_attr [V,Ca] of the caller -> contiguous float32 on the device, or ValueError"""
        V = self.pbr_mesh.vertices.shape[0]
        if v_attr is None:
            raise ValueError("%s(render_v_attr=True) needs v_attr [V, Ca]" % who)
        v_attr = torch.as_tensor(v_attr, dtype=torch.float32).to(self.device).contiguous()
        if v_attr.dim() != 2 or v_attr.shape[0] != V or v_attr.shape[1] < 1:
            raise ValueError("%s: v_attr is %s, the mesh has %d vertices: expected [%d, Ca >= 1]" % (who, tuple(v_attr.shape), V, V))
        return v_attr

    # flag of simple_rendering -> key of the returned dict, in the order the reference fills its dict
    _SCREEN_FLAGS = ("z_depth", "world_normal", "camera_normal", "world_position", "camera_position", "distance", "ray_direction", "cos_ray_normal",
                     "v_attr", "uv", "map_attr")
    _SCREEN_FLAGS_UNBUILT = ("render_voxel_attr", "render_voxel_network", "render_all_point_cloud", "render_visible_point_cloud", "render_map_network")

    def simple_rendering(self, c2ws, intrinsics, render_size, perspective=True, v_attr=None, map_attr=None, render_z_depth=False,
                         render_distance=False, render_world_normal=False, render_camera_normal=False, render_world_position=False,
                         render_camera_position=False, render_ray_direction=False, render_cos_ray_normal=False, render_v_attr=False,
                         render_uv=False, render_map_attr=False, background=None, grid_interpolate_mode="bilinear", enable_antialis=True, antialias=False,
                         **kwargs):
        """NVDiffRendererBase.simple_rendering (render/nvdiffrast/renderer_base.py:101-350) on the mesh of update_from_file / update_from_arrays: the
        buffers of a batch of cameras c2ws [B,4,4] / intrinsics [B,3,3] (normalised) on a screen of render_size (int or (H, W)).  One rasterisation
        per view (the loop mv_to_pcd uses), then every requested buffer of every view in ONE kernel launch (ops.screen_gbuffer).  Returns the
        reference's dict: 'mask' bool [B,H,W,1], 'alpha' float32 [B,H,W,1] and, per flag, 'world_normal' / 'camera_normal' / 'world_position' /
        'camera_position' / 'ray_direction' [B,H,W,3], 'z_depth' (the interpolated clip w) / 'distance' / 'cos_ray_normal' [B,H,W,1], 'uv' [B,H,W,2]
        in [-1,1], 'v_attr' [B,H,W,Ca] and 'map_attr' [B,H,W,sum C_i]; backgrounds as the reference fills them (-1 or 0).
        perspective replaces the reference's enable_perspective() / enable_orthogonal() state, as in infer and mv_to_pcd.  Vertex normals are
        pbr_mesh.vertex_normals, the vertex UVs the mesh's own.
        v_attr [V,Ca]: any per-vertex attribute (render_v_attr).  map_attr (render_map_attr): one map [Ht,Wt,C] or [1,Ht,Wt,C], row 0 at v = 0, or a
        tuple of up to four maps of sizes of their own, sampled at 'uv' and concatenated along the channels -- bit-identical to torch.cat of the
        single-map calls.  grid_interpolate_mode: 'bilinear' | 'nearest' are F.grid_sample(align_corners=False, zero padding), 'nvdiffrast' is
        dr.texture(uv * 0.5 + 0.5, filter_mode='linear') with its wrap boundary.  As in the reference, map_attr hangs under render_uv (:289-305):
        render_map_attr without render_uv is a ValueError here instead of being dropped.
        background (v_attr and map_attr only): None leaves the interpolated / sampled value on every pixel (uncovered pixels: 0, and the maps'
        sample at uv = (-1, -1)); a number or a tensor that broadcasts to the buffer ([C], [H,W,C], [B,H,W,C]) fills the uncovered pixels.
        enable_antialis is accepted and has no effect: without antialias=True alpha is the coverage mask, as on the turntable.
        antialias=True (this build's keyword, off by default) reproduces the reference's order of operations at enable_antialis=True (:143-336) with
        ops.antialias in the place of dr.antialias (this library's rule, DESIGN 8 "Silhouette antialiasing"; nvdiffrast's samples are not pinned):
        alpha = antialias(mask.float()); every buffer is blended with its background by torch.lerp(bg, x, alpha) with that alpha (v_attr / map_attr only
        when a background is given) and then antialiased with the ONE set of weights of the rasterisation (ops.antialias_weights once,
        ops.antialias_apply per buffer).  x is what the screen kernel computes, with 0 on the uncovered pixels, where dr.interpolate / F.normalize leave
        0.  As in the reference, with render_camera_position set 'distance' and 'ray_direction' are taken from the ALREADY antialiased camera position
        (:245-256), 'map_attr' is sampled at the un-antialiased uv (:299, :309-311), and 'mask' is unchanged.
        Refused, never dropped (NotImplementedError when set): render_voxel_attr / render_voxel_network (the reference's branch cannot execute: it
        permutes the 5-D voxel_attr.expand(batch_size, *shape[-4:]) with four indices, :203-204), render_all_point_cloud /
        render_visible_point_cloud (draw_mask hands the float pixel coordinates of discretize to torch.scatter as the index, :151-154, :28-36)
        and render_map_network (a callable of the caller's: apply it to 'uv').  Any other keyword is a TypeError.  render_v_attr without v_attr,
        render_map_attr without map_attr, more than four maps, or a v_attr whose first dimension is not V raise ValueError."""
        _refuse_unbuilt("simple_rendering", kwargs, self._SCREEN_FLAGS_UNBUILT)
        flags = dict(z_depth=render_z_depth, world_normal=render_world_normal, camera_normal=render_camera_normal, world_position=render_world_position,
                     camera_position=render_camera_position, distance=render_distance, ray_direction=render_ray_direction,
                     cos_ray_normal=render_cos_ray_normal, v_attr=render_v_attr, uv=render_uv, map_attr=render_map_attr)
        want = [k for k in self._SCREEN_FLAGS if flags[k]]
        m = self.pbr_mesh
        assert m is not None, "update_from_file first"
        _check_grid_interpolate_mode("simple_rendering", grid_interpolate_mode)
        if render_v_attr:
            v_attr = self._vertex_attr(v_attr, "simple_rendering")
        maps = ()
        if render_map_attr:
            if not render_uv:
                raise ValueError("simple_rendering(render_map_attr=True) samples the maps at 'uv': set render_uv=True as well (the reference renders "
                                 "map_attr under render_uv only)")
            if map_attr is None:
                raise ValueError("simple_rendering(render_map_attr=True) needs map_attr")
            maps = tuple(map_attr) if isinstance(map_attr, (tuple, list)) else (map_attr,)
            if not 1 <= len(maps) <= ops.SCREEN_MAX_MAPS:
                raise ValueError("simple_rendering: map_attr holds %d maps, 1 to %d are built" % (len(maps), ops.SCREEN_MAX_MAPS))
            maps = tuple(torch.as_tensor(t, dtype=torch.float32).to(self.device) for t in maps)
            maps = tuple((t[0] if t.dim() == 4 and t.shape[0] == 1 else t).contiguous() for t in maps)
            for t in maps:
                if t.dim() != 3 or min(t.shape) < 1:
                    raise ValueError("simple_rendering: a map is %s, expected [Ht, Wt, C] or [1, Ht, Wt, C]" % (tuple(t.shape),))
        with self._stage("view_raster"):
            mvp, c2ws_cpu, clip, _, rast = self._view_raster(c2ws, intrinsics, render_size, perspective)
        with self._stage("screen_gbuffer"):
            out = ops.screen_gbuffer(rast, m.faces, m.vertices, v_nrm=m.vertex_normals if _reads_vertex_normals(want) else None, v_uv=m.uvs_2d if render_uv else None,
                                     v_attr=v_attr if render_v_attr else None, maps=maps, c2ws=c2ws_cpu, want=["mask", "alpha"] + want,
                                     background=None if antialias else background, filter=grid_interpolate_mode,
                                     clip_w=clip[..., 3].contiguous() if render_z_depth else None)
        if antialias:      # the launch above ran without the background: the blend below needs the raw value on the uncovered pixels as well
            with self._stage("antialias"):
                out = self._antialias_buffers(out, want, rast, clip, background)
        out["mask"] = out["mask"].bool()[..., None]
        return out

    # buffer -> the background the reference blends it with at enable_antialis=True (renderer_base.py:165-303)
    _SCREEN_FILL = dict(z_depth=0.0, world_normal=-1.0, camera_normal=-1.0, world_position=-1.0, camera_position=0.0, distance=0.0, ray_direction=-1.0,
                        cos_ray_normal=-1.0, uv=-1.0)

    def _antialias_buffers(self, out, want, rast, clip, background):
        """simple_rendering(antialias=True): the buffers of the antialias=False launch -> the reference's at enable_antialis=True.  The kernel's covered
        pixels are the raw values x; its uncovered pixels are put back to the 0 that dr.interpolate / F.normalize leave there, then lerp and stencil."""
        m = self.pbr_mesh
        weights = ops.antialias_weights(rast, clip, m.faces, m.edge_opposites)
        covered = out["mask"].bool()[..., None]
        alpha = ops.antialias_apply(out["alpha"], weights)
        res = {"mask": out["mask"], "alpha": alpha}

        def blend(x, fill):
            return ops.antialias_apply(torch.lerp(torch.full_like(x, fill), x, alpha).contiguous(), weights)

        for k in want:
            x = out[k]
            if k in ("v_attr", "map_attr"):
                if background is None:      # no pre-blend: the value as computed on every pixel
                    res[k] = ops.antialias_apply(x, weights)
                    continue
                bg = torch.full_like(x, float(background)) if isinstance(background, (int, float)) else \
                    torch.as_tensor(background, dtype=torch.float32).to(x.device).expand_as(x)
                res[k] = ops.antialias_apply(torch.lerp(bg, x, alpha).contiguous(), weights)
                continue
            x = torch.where(covered, x, torch.zeros_like(x))
            # `want` follows _SCREEN_FLAGS, which lists camera_position BEFORE distance and ray_direction: with render_camera_position set its
            # antialiased buffer is in `res` by now and the two are taken from it, as the reference overwrites its local (:245-256); without it
            # they keep the kernel's raw value (:243, :250, :256)
            assert self._SCREEN_FLAGS.index("camera_position") < min(self._SCREEN_FLAGS.index("distance"), self._SCREEN_FLAGS.index("ray_direction"))
            if k in ("distance", "ray_direction") and "camera_position" in res:
                cp = res["camera_position"]
                x = torch.norm(cp, p=2, dim=-1, keepdim=True) if k == "distance" else torch.nn.functional.normalize(cp, dim=-1)
            res[k] = blend(x, self._SCREEN_FILL[k])
        return res

    def geometry_rendering(self, c2ws, intrinsics, render_size, render_all_point_cloud=False, render_visible_point_cloud=False, render_z_depth=True,
                           render_distance=True, render_world_normal=True, render_camera_normal=True, render_world_position=True,
                           render_camera_position=True, render_ray_direction=True, render_cos_ray_normal=True, render_uv=True, background=None, antialias=False, **kwargs):
        """NVDiffRendererBase.geometry_rendering (renderer_base.py:745-780): simple_rendering with every geometry buffer on by default and neither v_attr nor
        map_attr.  The two point-cloud flags default to False, what simple_rendering builds (the reference's True); True raises as it does there, and so does
        every other keyword simple_rendering refuses."""
        return self.simple_rendering(c2ws, intrinsics, render_size, render_all_point_cloud=render_all_point_cloud,
                                     render_visible_point_cloud=render_visible_point_cloud, render_z_depth=render_z_depth, render_distance=render_distance,
                                     render_world_normal=render_world_normal, render_camera_normal=render_camera_normal,
                                     render_world_position=render_world_position, render_camera_position=render_camera_position,
                                     render_ray_direction=render_ray_direction, render_cos_ray_normal=render_cos_ray_normal, render_v_attr=False,
                                     render_uv=render_uv, render_map_attr=False, background=background, antialias=antialias, **kwargs)

    def vertex_rendering(self, v_rgb, c2ws, intrinsics, render_size, render_rgb=True, render_all_point_cloud=False, render_visible_point_cloud=False,
                         render_z_depth=False, render_distance=False, render_world_normal=False, render_camera_normal=False, render_world_position=False,
                         render_camera_position=False, render_ray_direction=False, render_cos_ray_normal=False, background=None, antialias=False, **kwargs):
        """NVDiffRendererBase.vertex_rendering (renderer_base.py:782-820): simple_rendering of the per-vertex colour v_rgb [V,C]; 'rgb' is 'v_attr'."""
        out = self.simple_rendering(c2ws, intrinsics, render_size, v_attr=v_rgb, render_all_point_cloud=render_all_point_cloud,
                                    render_visible_point_cloud=render_visible_point_cloud, render_z_depth=render_z_depth, render_distance=render_distance,
                                    render_world_normal=render_world_normal, render_camera_normal=render_camera_normal,
                                    render_world_position=render_world_position, render_camera_position=render_camera_position,
                                    render_ray_direction=render_ray_direction, render_cos_ray_normal=render_cos_ray_normal, render_v_attr=render_rgb,
                                    render_uv=False, render_map_attr=False, background=background, antialias=antialias, **kwargs)
        if render_rgb:
            out["rgb"] = out["v_attr"]
        return out

    def uv_rendering(self, map_Kd, c2ws, intrinsics, render_size, render_rgb=True, render_all_point_cloud=False, render_visible_point_cloud=False,
                     render_z_depth=False, render_distance=False, render_world_normal=False, render_camera_normal=False, render_world_position=False,
                     render_camera_position=False, render_ray_direction=False, render_cos_ray_normal=False, background=None, antialias=False, **kwargs):
        """NVDiffRendererBase.uv_rendering (renderer_base.py:822-860): simple_rendering of the texture map_Kd ([Ht,Wt,C], [1,Ht,Wt,C] or a tuple of maps) with
        'uv' always on, as in the reference; 'rgb' is 'map_attr'."""
        out = self.simple_rendering(c2ws, intrinsics, render_size, map_attr=map_Kd, render_all_point_cloud=render_all_point_cloud,
                                    render_visible_point_cloud=render_visible_point_cloud, render_z_depth=render_z_depth, render_distance=render_distance,
                                    render_world_normal=render_world_normal, render_camera_normal=render_camera_normal,
                                    render_world_position=render_world_position, render_camera_position=render_camera_position,
                                    render_ray_direction=render_ray_direction, render_cos_ray_normal=render_cos_ray_normal, render_v_attr=False,
                                    render_uv=True, render_map_attr=render_rgb, background=background, antialias=antialias, **kwargs)
        if render_rgb:
            out["rgb"] = out["map_attr"]
        return out

    GLOBAL_INTERPOLATE_MODES = ("nearest", "linear", "barycentric")

    def global_inverse_rendering(self, image_attr, c2ws, intrinsics, render_size, texture_size, image_mask=None, image_mask_exclude_boundary=True,
                                 texture_attr=None, texture_mask=None, ray_angle_degree_threshold=None, normal_angle_degree_threshold=None,
                                 grid_interpolate_mode="linear", inpainting_occlusion=True, n_neighbors=10, n_iters_max=1000, perspective=True, **kwargs):
        """NVDiffRendererBase.global_inverse_rendering (render/nvdiffrast/renderer_base.py:562-743) on the mesh of update_from_file / update_from_arrays:
        the views image_attr [B,H,W,C] of the cameras c2ws [B,4,4] / intrinsics [B,3,3] baked into an atlas of texture_size (int or (H, W)) from scattered
        samples.  Every view pixel that passes the sample mask -- coverage, its four neighbours covered (image_mask_exclude_boundary; the image wraps
        round, as torch.roll), normal_angle_degree_threshold on the interpolated camera-space normal's z, ray_angle_degree_threshold on the dot of
        the interpolated direction and normal, image_mask [B,H,W,1] -- is a sample (its UV, its colour) (ops.view_samples, one launch).  The texels
        predicted are those on a face that get_visible_faces(method='rays') reports for some view, minus texture_mask; each takes the colour of its
        nearest sample in UV ('nearest' = scipy's NearestNDInterpolator: ops.knn_gather with k = 1 on a zero third coordinate; ties go to the lower
        sample index).  inpainting_occlusion then fills the covered texels no view sees along the SURFACE: k = n_neighbors nearest covered texels in
        3-D (ops.knn_gather on the set itself), weight = L1-normalised reciprocal distance times the cosine between the normals (arXiv 2411.02336
        section 3.2), one Jacobi sweep per step (ops.knn_inpaint) until a step fills nothing or n_iters_max; a texel with k - 1 or more unknown
        neighbours waits, and one that never qualifies keeps colour 0 and stays out of map_mask.  The reference's arithmetic is mirrored where it is
        odd (duplicate positions give NaN, which the closing nan_to_num turns into 0).
        Returns the reference's dict: map_attr [Ht,Wt,C], map_alpha [Ht,Wt,1] (the atlas coverage), map_mask bool [Ht,Wt,1] (predicted or given), samples_u
        [Ns,2], samples_v [Ns,C], predicts_u [Np,2], predicts_v [Np,C], samples_x [M,6] / samples_y [M,C] (the covered texels' position + normal and
        final colour; None without inpainting_occlusion), tex_to_pos [B,H,W,2], tex_to_pos_cam [B,H,W,6], world_to_tex [Ht,Wt,6].  Atlas row 0 is v = 0.
        texture_attr [Ht,Wt,C] / texture_mask [Ht,Wt,1] (both or neither): the texels of texture_mask keep texture_attr and are not predicted.
        perspective replaces the reference's enable_perspective() / enable_orthogonal() state.
        grid_interpolate_mode keeps the reference's default 'linear', which -- like 'barycentric' -- is a scipy Delaunay interpolator on the host and is
        refused (NotImplementedError): pass 'nearest'.  An unknown mode, texture_attr without texture_mask (or the reverse), n_neighbors outside 1..32 or
        above the number of covered texels, and a call in which no pixel passes the sample mask raise ValueError; an unknown keyword is a TypeError, `antialias` among them (not wired here)."""
        who = "global_inverse_rendering"
        for k_ in kwargs:
            raise TypeError("%s() got an unexpected keyword argument %r" % (who, k_))
        if grid_interpolate_mode not in self.GLOBAL_INTERPOLATE_MODES:
            raise ValueError("%s(grid_interpolate_mode=%r): one of %s" % (who, grid_interpolate_mode, ", ".join(self.GLOBAL_INTERPOLATE_MODES)))
        if grid_interpolate_mode != "nearest":
            raise NotImplementedError("%s(grid_interpolate_mode=%r) is not built (scipy's Delaunay interpolators on the host): pass grid_interpolate_mode='nearest'"
                                      % (who, grid_interpolate_mode))
        if (texture_attr is None) != (texture_mask is None):
            raise ValueError("%s: texture_attr and texture_mask come together" % who)
        if not 1 <= int(n_neighbors) <= ops.KNN_INPAINT_K_MAX:
            raise ValueError("%s(n_neighbors=%r): 1 to %d" % (who, n_neighbors, ops.KNN_INPAINT_K_MAX))
        m, dev = self.pbr_mesh, self.device
        assert m is not None, "update_from_file first"
        image_attr = torch.as_tensor(image_attr, dtype=torch.float32).to(dev)
        Ht, Wt = (texture_size, texture_size) if isinstance(texture_size, int) else texture_size
        with self._stage("view_raster"):
            _, c2ws_cpu, _, _, rast = self._view_raster(c2ws, intrinsics, render_size, perspective)
        B, H, W = rast.shape[:3]
        if image_attr.dim() != 4 or tuple(image_attr.shape[:3]) != (B, H, W) or not 1 <= image_attr.shape[3] <= ops.CHANNELS_MAX:
            raise ValueError("%s: image_attr is %s, expected [%d, %d, %d, 1 <= C <= %d]" % (who, tuple(image_attr.shape), B, H, W, ops.CHANNELS_MAX))
        Cc = image_attr.shape[3]
        rast2d = self._uv_raster(int(Ht), int(Wt))
        covered = rast2d[..., 3] > 0
        with self._stage("visible_faces"):
            seen = self._visible_faces(c2ws_cpu, perspective, "rays", None, 0).bool().any(dim=0)
        predicts_mask = covered & seen[(rast2d[..., 3].long() - 1).clamp_(min=0)]
        if texture_mask is not None:
            texture_attr = torch.as_tensor(texture_attr, dtype=torch.float32).to(dev)
            texture_mask = torch.as_tensor(texture_mask).to(dev).bool()
            if tuple(texture_attr.shape) != (Ht, Wt, Cc) or tuple(texture_mask.shape) != (Ht, Wt, 1):
                raise ValueError("%s: texture_attr is %s and texture_mask %s, expected %s and %s" % (who, tuple(texture_attr.shape), tuple(texture_mask.shape),
                                                                                                     (Ht, Wt, Cc), (Ht, Wt, 1)))
            predicts_mask = predicts_mask & ~texture_mask[..., 0]
        with self._stage("samples"):
            v_pos_cam, v_nrm_cam = ops._camera_arrays(m.vertices, m.vertex_normals, c2ws_cpu, B, True, True, None, None)
            tex_to_pos, tex_to_pos_cam, smask = ops.view_samples(rast, m.faces, m.uvs_2d, v_pos_cam, v_nrm_cam, image_mask_exclude_boundary,
                                                                 normal_angle_degree_threshold, ray_angle_degree_threshold, image_mask)
            world_to_tex = ops.interpolate(torch.cat([m.vertices, m.vertex_normals], dim=-1).contiguous(), rast2d, m.faces)
            smask = smask.bool()
            samples_u, samples_v = tex_to_pos[smask], image_attr[smask]
            # undiscretize (camera/conversion.py:183-197): the texel centres in [-1, 1], x first
            gx = (torch.arange(Wt, dtype=torch.float32, device=dev) + 0.5) / Wt * 2.0 - 1.0
            gy = (torch.arange(Ht, dtype=torch.float32, device=dev) + 0.5) / Ht * 2.0 - 1.0
            tex_to_tex = torch.stack([gx[None, :].expand(Ht, Wt), gy[:, None].expand(Ht, Wt)], dim=-1)
            predicts_u = tex_to_tex[predicts_mask]
        if samples_u.shape[0] == 0:
            raise ValueError("%s: no pixel of any view passes the sample mask" % who)
        with self._stage("nearest"):
            if predicts_u.shape[0] > 0:
                z = lambda t: torch.cat([t, torch.zeros_like(t[:, :1])], dim=-1).contiguous()
                predicts_v = ops.knn_gather(z(samples_u), z(predicts_u), 1, src_attr=samples_v.contiguous())
            else:
                predicts_v = torch.zeros(0, Cc, dtype=torch.float32, device=dev)
        map_attr = torch.zeros(Ht, Wt, Cc, dtype=torch.float32, device=dev)
        map_attr[predicts_mask] = predicts_v
        map_mask = predicts_mask & ~torch.isnan(map_attr).any(dim=-1)
        map_attr = torch.nan_to_num(map_attr, nan=0.0).clamp_(0.0, 1.0)
        if texture_mask is not None:
            map_attr = torch.where(texture_mask, texture_attr, map_attr)
            map_mask = covered & (map_mask | texture_mask[..., 0])
        samples_x = samples_y = None
        self.last = {"rast2d": rast2d, "view_mask": smask, "inpaint_steps": 0}
        if inpainting_occlusion:
            samples_x = world_to_tex[covered]
            M = samples_x.shape[0]
            if M < int(n_neighbors):
                raise ValueError("%s(n_neighbors=%d): the atlas covers %d texels only" % (who, n_neighbors, M))
            with self._stage("knn"):
                pos = samples_x[:, :3].contiguous()
                _, idx, d2 = ops.knn_gather(pos, pos, int(n_neighbors), want_index=True)
            with self._stage("propagation"):
                samples_y, _, steps = ops.knn_inpaint(idx, d2, samples_x[:, 3:].contiguous(), map_attr[covered], (~map_mask)[covered].to(torch.uint8),
                                                      n_iters_max=n_iters_max)
            self.last["inpaint_steps"] = steps
            map_attr = torch.zeros_like(map_attr)
            map_attr[covered] = samples_y
            map_attr = torch.nan_to_num(map_attr, nan=0.0).clamp_(0.0, 1.0)
        return {"map_attr": map_attr, "map_alpha": covered[..., None].to(torch.float32), "map_mask": map_mask[..., None], "samples_u": samples_u,
                "samples_v": samples_v, "predicts_u": predicts_u, "predicts_v": predicts_v, "samples_x": samples_x, "samples_y": samples_y,
                "tex_to_pos": tex_to_pos, "tex_to_pos_cam": tex_to_pos_cam, "world_to_tex": world_to_tex}

    def compute_uv_mask(self, texture_size=2048):
        """Mesh.compute_uv_mask (mesh/structure.py:786-799): the atlas coverage, bool [H,W,1]"""
        return self.simple_inverse_rendering(None, texture_size, enable_antialis=False)["mask"][0]

    def export_uv_maps(self, save_dir, texture_size=2048):
        """uv_mask.png (L), uv_position.png and uv_normal.png (x * 0.5 + 0.5, background -1 -> 0) of the atlas, rows flipped so that the images
        lie like the baked texture (TexturedMesh.texture: row 0 is v = 1).  Returns the three paths."""
        from PIL import Image
        out = self.simple_inverse_rendering(None, texture_size, render_world_normal=True, render_world_position=True)
        os.makedirs(save_dir, exist_ok=True)
        level = int(os.environ.get("UTX_PNG_LEVEL", "1"))
        paths = [os.path.join(save_dir, n) for n in ("uv_mask.png", "uv_position.png", "uv_normal.png")]
        Image.fromarray(out["mask"][0, ..., 0].flip(0).to(torch.uint8).mul(255).cpu().numpy()).save(paths[0], compress_level=level)
        for key, path in (("world_position", paths[1]), ("world_normal", paths[2])):
            ndc = (out[key][0] * 0.5 + 0.5).contiguous()
            Image.fromarray(ops.to_u8(ndc, flip=True).cpu().numpy()).save(path, compress_level=level)
        return paths

    def infer(self, blank_mesh, c2ws, intrinsics, image_attrs, H=512, W=512, H2D=2048, W2D=2048, perspective=True,
              grad_norm_threhold=0.20, ray_normal_angle_threhold=115.0, grid_interpolate_mode="torch", method="reproject",
              kdtree_n_neighbors=32, kdtree_n_neighbors_visiable=1, kdtree_n_neighbors_invisiable=32, kdtree_method="order_mean",
              kdtree_inpainting=False, reproject_method="lens", reproject_kernel_size_boundary=3, reproject_kernel_size_boundary_blur=3,
              reproject_kernel_size_blur=5, reproject_inpainting=False, filt_gradient_points=True, return_layers=False, **unused):
        """renderer_inverse.py:635-726.  method='reproject' is bake_mv_to_uv_reproject_blur (the pipeline's path),
        method='kdtree' bake_mv_to_uv_kdtree ('order_mean' | 'mean' | 'mvpaint'); *_inpainting=True routes the unseen texels
        through the registered query field (the LTM hook) instead of the nearest-neighbour fill; filt_gradient_points adds
        the gradient / facing filter to the view masks.  Colours: 3 channels (rgb) or 9 (PBR stack: albedo, metallic-roughness, bump) for both methods;
        nine channels return a TexturedMesh with .metallic_roughness and .bump, and with method='reproject' refuse return_layers=True (that path has no
        per-view colour layers).
        grid_interpolate_mode 'torch' | 'pytorch' samples the views as grid_sample (zero padding), 'nvdiff' | 'nvdiffrast' as nvdiffrast's
        linear dr.texture (wrap boundary).  reproject_method 'lens' | 'gaussian' picks the seam blur; the seam is the winner boundary within
        reproject_kernel_size_boundary // 2, dilated by reproject_kernel_size_boundary_blur // 2 (both radii <= 15), and 'gaussian' blurs it with
        torchvision's gaussian_blur at reproject_kernel_size_blur (odd, <= 31; 'lens' ignores the size, as the reference does)."""
        assert method in ("kdtree", "reproject")
        _check_channels(image_attrs.shape)
        stack = method == "reproject" and image_attrs.shape[-1] != 3      # the 9-channel path: colour gathered from the winning view only
        if stack and return_layers:
            raise NotImplementedError("infer(return_layers=True) with %d channels and method='reproject': that path gathers colour from the winning view "
                                      "only, the per-view colour layers do not exist" % image_attrs.shape[-1])
        t_host0 = time.perf_counter()
        # keyword arguments of the reference's signature (renderer_inverse.py:635-659) that this build fixes at the value the pipeline uses: anything else is
        # refused, not dropped
        fixed = dict(return_mv_reproject_uv=False)
        for k_, v_ in unused.items():
            if k_ not in fixed:
                raise TypeError("infer() got an unexpected keyword argument %r" % k_)
            if v_ != fixed[k_]:
                raise NotImplementedError("infer(%s=%r): only %r (the pipeline's value) is built" % (k_, v_, fixed[k_]))
        assert grid_interpolate_mode in ("torch", "pytorch", "nvdiff", "nvdiffrast")      # uv_to_pcd, :260
        sample = "nvdiff" if grid_interpolate_mode in ("nvdiff", "nvdiffrast") else "grid"
        assert reproject_method in ("gaussian", "lens")                                    # bake_mv_to_uv_reproject_blur, :587
        if method == "reproject":
            _check_seam_sizes(reproject_kernel_size_boundary, reproject_kernel_size_boundary_blur)
            if reproject_method == "gaussian":
                _check_gaussian_ksize(reproject_kernel_size_blur)
        assert len(self.index) == image_attrs.shape[0] == torch.as_tensor(c2ws).shape[0]
        m = self.pbr_mesh
        n = image_attrs.shape[0]
        dev = self.device
        image_attrs = torch.as_tensor(image_attrs, dtype=torch.float32).to(dev)
        with self._stage("view_raster"):
            mv = self.mv_to_pcd(c2ws, intrinsics, (H, W), perspective=perspective, grad_norm_threhold=grad_norm_threhold,
                                ray_normal_angle_threhold=ray_normal_angle_threhold, filt_gradient_points=filt_gradient_points,
                                want_points=(method == "kdtree"))
        # the alpha channel the texels sample is mask_visiable (uv_to_pcd(alpha_attrs=alpha_visiable), :661-670)
        images = None if stack else torch.cat([image_attrs[..., :3], mv["alpha"][..., None]], dim=-1).contiguous()
        _, c2ws_cpu = self._mvp(c2ws, intrinsics, perspective)
        # ray model per view (uv_to_pcd, :279-284): perspective -- from the camera centre to each texel's surface point; orthographic -- along -z of the camera
        eyes = c2ws_cpu[:, :3, 3].contiguous().to(dev) if perspective else None
        dirs = None if perspective else (-c2ws_cpu[:, :3, 2]).contiguous().to(dev)
        rast2d = self._uv_raster(H2D, W2D)
        from .distributed import view_range
        rank, world = self.view_shard
        v0, v1, per = view_range(rank, world, n)
        # the back-projection kernel writes EVERY texel of the views it is given; only a view shard (world > 1) leaves layers to others, and those start as zeros
        alloc = torch.zeros if (world > 1 or v1 - v0 < n) else torch.empty
        color = None if stack else alloc(n, H2D, W2D, 3, dtype=torch.float32, device=dev)
        rayvis = alloc(n, H2D, W2D, dtype=torch.uint8, device=dev)
        alphaok = alloc(n, H2D, W2D, dtype=torch.uint8, device=dev)
        with self._stage("bvh_build"):
            bvh = m.optix
        vndc = mv["ndc"].contiguous()
        if v1 > v0:
            with self._stage("backproject"):
                if stack:
                    ops.backproject_vis(rast2d, m.vertices, m.faces, m.normals, vndc, dirs, mv["alpha"].contiguous(), bvh,
                                        angle_deg=ray_normal_angle_threhold, view_begin=v0, view_count=v1 - v0, out=(rayvis, alphaok), eyes=eyes,
                                        sample=sample)
                else:
                    ops.backproject(rast2d, m.vertices, m.faces, m.normals, vndc, dirs, images, bvh,
                                    angle_deg=ray_normal_angle_threhold, view_begin=v0, view_count=v1 - v0, out=(color, rayvis, alphaok), eyes=eyes,
                                    sample=sample)
        with self._stage("dilate_visibility"):
            vis = ops.dilate_visibility(rayvis, alphaok, rast2d)
        if world > 1:
            with self._stage("all_gather"):          # the one exchange step of the path
                if stack:
                    from .distributed import gather_view_images
                    vis = gather_view_images(vis, rank, world, group=self.process_group)      # the u8 visibility layers only
                else:
                    color, vis = self._gather_layers(color, vis, per, n)
        mask_u8 = (rast2d[..., 3] > 0).to(torch.uint8).contiguous()
        winner = seam = None
        if method == "reproject":
            with self._stage("composite"):
                if stack:
                    winner = ops.composite_winner(vis, self.index)
                else:
                    atlas, winner = ops.composite(color, vis, self.index)
            with self._stage("seam_mask"):
                seam = ops.seam_mask(winner, rast2d, reproject_kernel_size_boundary, reproject_kernel_size_boundary_blur)
            if stack:
                with self._stage("gather_winner"):
                    atlas = ops.gather_winner(rast2d, m.faces, vndc, image_attrs.contiguous(), winner, sample=sample)
            with self._stage("nn_fill"):
                pos = ops.interpolate(m.vertices, rast2d, m.faces)
                if reproject_inpainting:
                    self._fill_unseen(atlas, (winner >= 0).to(torch.uint8), rast2d[..., 3] > 0, pos, True)
                else:
                    ops.nn_fill(atlas, winner, rast2d, pos)
            if reproject_method == "gaussian":
                with self._stage("gaussian_blur_seam"):
                    baked = ops.gaussian_blur_seam(atlas, seam, reproject_kernel_size_blur)
            else:
                with self._stage("lens_blur_seam"):
                    baked = ops.lens_blur_seam(atlas, seam)
        else:
            with self._stage("kdtree_bake"):
                pos2d = ops.interpolate(m.vertices, rast2d, m.faces)
                baked = self._bake_kdtree(mv, image_attrs.contiguous(), vis, rast2d, pos2d,
                                          kdtree_method, kdtree_n_neighbors, kdtree_n_neighbors_visiable, kdtree_n_neighbors_invisiable,
                                          kdtree_inpainting)
        with self._stage("pull_push"):
            color_2d = ops.pull_push(baked, mask_u8)
        with self._stage("to_u8"):
            # tensor_to_image + FLIP_TOP_BOTTOM (link_pbr_to_mesh.py:17 / :46-48); nine channels: albedo 0:3, metallic-roughness 3:6, bump 6:9 (:716-721)
            texs = [ops.to_u8(color_2d[..., c:c + 3].contiguous(), flip=True) for c in range(0, color_2d.shape[-1], 3)]
            tex = texs[0]
        self.host_enqueue_ms = (time.perf_counter() - t_host0) * 1e3      # the host's wall time up to the last enqueue.  NOT free of device waits when the tree is fresh: the first utx_backproject behind utx_bvh_build_ws blocks in
        # hipEventSynchronize(depth_ready) until the build -- and everything queued in front of it -- has run (the depth picks the traversal on the host), so on a new mesh this figure
        # contains that GPU time; on a cached tree (DeviceMesh.optix, the benchmark's later iterations) it is enqueue time only.  The copies below wait for the GPU
        extra = [t.cpu().numpy() for t in texs[1:3]] if len(texs) == 3 else [None, None]
        textured = TexturedMesh(m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.uvs01, tex.cpu().numpy(), *extra)
        self.last = {"rast2d": rast2d, "winner": winner, "seam": seam, "atlas_prefill": baked, "view_mask": mv["mask_visiable"]}
        out = (textured, vis.bool()[..., None], (rast2d[..., 3] > 0)[None, ..., None], color_2d[None])
        if return_layers:
            return out + (color, vis)
        return out

    def _gather_layers(self, color, vis, per, n):
        """ONE all-gather of the per-view layers (texturetools/distributed.py)."""
        from .distributed import gather_view_layers
        rank, world = self.view_shard
        return gather_view_layers(color, vis, rank, world, group=self.process_group)
