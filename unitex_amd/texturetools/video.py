"""VideoExporter.export_condition -- geometry-condition render (alpha / world-position 'ccm' / world-normal
grids) that feeds the DiT (reference: TextureTools/texturetools/video/export_nvdiffrast_video.py:900-999 on
top of NVDiffRendererBase.simple_rendering, render/nvdiffrast/renderer_base.py:101-200).

HIP path: clip transform -> rasterise per view -> interpolate vertex normals / positions -> fused shade +
uint8 conversion kernel; orthographic box views (the pipeline's) or, as the reference's defaults, a perspective
camera (fov_deg) and / or the orbit ring (orbit=True).  export_orbit_video (video/export_nvdiffrast_video.py:141-256): per frame clip transform ->
perspective raster -> fused UV interpolation + bilinear texture fetch + background composite (utx_texture_shade);
the geometry video types (world / camera normal, world / camera position, z_depth, distance) swap that last kernel for the fused geometry-buffer
shade (utx_gbuffer_shade; alpha = coverage, dr.antialias is not wired here); frames are muxed on the host (Motion-JPEG in an MP4 container, or GIF -- there is
no video encoder in this image)."""
import io
import math
import os
import struct

import numpy as np
import torch
from PIL import Image

from . import camera, meshes, ops


def _vertex_normals(verts, faces, weighting="area"):
    """per-vertex normals, float64 on the host (mesh preparation, not hot path).

    weighting="area": face cross products splatted to the vertices, normalised; vertices with a zero sum (unreferenced /
      degenerate) get (0, 0, 1) -- Mesh._compute_vertex_normal (mesh/structure.py:522-548), the reference's own code,
      pinned by fixture G9.
    weighting="angle": unit face normals weighted by the corner angle at the vertex, normalised -- what trimesh's
      `vertex_normals` computes [3p, trimesh==3.20.2, restated from its published algorithm; unpinned], which is what the
      reference's forward render actually consumes when trimesh is installed (Mesh.from_trimesh, structure.py:355-356)."""
    v, f = verts.double(), faces.long()
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    c = torch.linalg.cross(p1 - p0, p2 - p0, dim=-1)
    n = torch.zeros_like(v)
    if weighting == "area":
        for k in range(3):
            n.index_add_(0, f[:, k], c)
        n = torch.where((n * n).sum(-1, keepdim=True) > 1e-20, n, torch.tensor([0.0, 0.0, 1.0], dtype=n.dtype))
    elif weighting == "angle":
        fn = torch.nn.functional.normalize(c, dim=-1)
        unit = lambda a: torch.nn.functional.normalize(a, dim=-1)
        corners = ((p0, p1, p2), (p1, p2, p0), (p2, p0, p1))
        for k, (a, b, d) in enumerate(corners):
            ang = torch.arccos(torch.clamp((unit(b - a) * unit(d - a)).sum(-1), -1.0, 1.0))
            n.index_add_(0, f[:, k], fn * ang[:, None])
    else:
        raise ValueError("weighting must be 'area' or 'angle'")
    return torch.nn.functional.normalize(n, dim=-1).float().contiguous()


def condition_cameras(n_views, n_rows, n_cols, scale=0.85, fov_deg=49.1, perspective=False, orbit=True):
    """(c2ws [n_views,4,4], intrinsics [3,3]) of export_condition (export_nvdiffrast_video.py:921-943): the orbit ring or the box views, a
    perspective camera of fov_deg or an orthographic one of `scale`."""
    if orbit:            # n_views + 1 cameras on the ring at radius 2.8, the last (= the first, 360 degrees on) dropped (export_nvdiffrast_video.py:921-922)
        c2ws = camera.generate_orbit_views_c2ws(n_views + 1, radius=2.8, height=0.0, theta_0=0.0, degree=True)[:n_views]
    elif n_views == 8:   # BASELINE configs[4]: the six axis views + two upper diagonals (camera.generate_views_c2ws; builder-defined)
        c2ws, _ = camera.generate_views_c2ws(8, radius=2.8)
    else:
        c2ws = camera.generate_box_views_c2ws(radius=2.8)
        sel = {1: [0], 2: [0, 2], 4: [0, 1, 2, 3], 6: [0, 1, 4, 2, 3, 5] if (n_rows, n_cols) == (2, 3) else list(range(6))}[n_views]
        c2ws = c2ws[sel]
    if perspective:      # export_nvdiffrast_video.py:938-943
        intrinsics = camera.generate_intrinsics(fov_deg, fov_deg, fov=True, degree=True)
    else:
        intrinsics = camera.generate_intrinsics(scale, scale, fov=False, degree=False)
    return c2ws, intrinsics


class VideoExporter:
    def __init__(self, device="cuda", normal_weighting="angle", view_shard=(0, 1), process_group=None):
        self.device = torch.device(device if device != "cuda" else "cuda:%d" % torch.cuda.current_device())
        self.normal_weighting = normal_weighting      # see _vertex_normals: "angle" = trimesh semantics
        self.view_shard = view_shard                  # (rank, world): this rank renders its block of the condition views,
        self.process_group = process_group            # one all-gather of the uint8 images completes the grids on every rank

    def export_condition(self, mesh_path, geometry_scale=1.0, n_views=4, n_rows=2, n_cols=2, H=512, W=512, scale=0.85,
                         fov_deg=49.1, perspective=False, orbit=True, background=None, return_info=False,
                         return_image=True, return_mesh=False, return_camera=False):
        assert n_views == n_rows * n_cols, "Value Error: (n_views, n_rows, n_cols)=%s" % ((n_views, n_rows, n_cols),)
        if return_info or return_mesh or not return_image:
            # export_nvdiffrast_video.py:948-975: the set-up only / float arrays / the loaded mesh object -- forms the texture pipeline never asks for
            # (pipeline.py:200-216); the fused shade kernel produces the uint8 images directly
            raise NotImplementedError("export_condition: only return_image=True (+ return_camera) is built")
        if isinstance(mesh_path, str):
            # the reference renders the conditions from the RAW input mesh (pipeline.py:573 -> export_nvdiffrast_video.py:900-999), any format its
            # loader reads; here .obj (shared positions: normals are smoothed over position indices) and .glb
            if mesh_path.lower().endswith(".obj"):
                verts, faces, _, _ = meshes.load_obj(mesh_path)
            else:
                verts, faces, _, _ = meshes.load_mesh(mesh_path)
        else:
            verts, faces = mesh_path
        verts = torch.as_tensor(verts, dtype=torch.float32)
        faces = torch.as_tensor(faces, dtype=torch.int32)
        # scale_to_bbox(scale=geometry_scale): largest bbox side -> 2*scale, centred (mesh/structure.py:290-303, A7)
        lo, hi = verts.min(0).values, verts.max(0).values
        s = (hi - lo).max() / (2.0 * geometry_scale)
        verts = ((verts - 0.5 * (lo + hi)) / s).contiguous()
        c2ws, intrinsics = condition_cameras(n_views, n_rows, n_cols, scale=scale, fov_deg=fov_deg, perspective=perspective, orbit=orbit)
        bg = camera.parse_color(background)
        dev = self.device
        vd, fd = verts.to(dev), faces.to(dev).contiguous()
        nrm = _vertex_normals(verts, faces, self.normal_weighting).to(dev)
        mvp = torch.matmul(camera.intr_to_proj(intrinsics, perspective=perspective), camera.c2w_to_w2c(c2ws)).to(dev).contiguous()
        clip, _ = ops.transform_points(vd, mvp, want_ndc=False)
        from .distributed import gather_view_images, view_range
        rank, world = self.view_shard
        v0, v1, _ = view_range(rank, world, n_views)
        rasts, ns, ps = [], [], []
        for v in range(v0, v1):
            r = ops.rasterize(clip[v].contiguous(), fd, H, W)
            rasts.append(r)
            ns.append(ops.interpolate(nrm, r, fd))
            ps.append(ops.interpolate(vd, r, fd))
        bgv = bg.tolist() if bg is not None else [0.0, 0.0, 0.0]
        stack = torch.zeros(n_views, H, W, 7, dtype=torch.uint8, device=dev)
        if v1 > v0:
            n8, c8, a8 = ops.condition_shade(torch.stack(rasts), torch.stack(ns), torch.stack(ps), bgv)
            stack[v0:v1, ..., 0:3], stack[v0:v1, ..., 3:6], stack[v0:v1, ..., 6] = n8, c8, a8
        if world > 1:
            stack = gather_view_images(stack, rank, world, group=self.process_group)
        normal_u8, ccm_u8, alpha_u8 = stack[..., 0:3].contiguous(), stack[..., 3:6].contiguous(), stack[..., 6].contiguous()

        def grid(t):
            a = t.cpu().numpy()
            if a.ndim == 3:
                return a.reshape(n_rows, n_cols, H, W).transpose(0, 2, 1, 3).reshape(n_rows * H, n_cols * W)
            return a.reshape(n_rows, n_cols, H, W, 3).transpose(0, 2, 1, 3, 4).reshape(n_rows * H, n_cols * W, 3)
        results = {"alpha": Image.fromarray(grid(alpha_u8), mode="L"), "ccm": Image.fromarray(grid(ccm_u8), mode="RGB"),
                   "normal": Image.fromarray(grid(normal_u8), mode="RGB")}
        if return_camera:
            results.update({"c2ws": c2ws, "intrinsics": intrinsics, "perspective": perspective})
        return results


    def export_orbit_video(self, mesh_obj, video_path, n_frames=120, enhance_mode=None, perspective=True, video_type="rgb",
                           save_frames=False, save_grid=False, save_cover=False, save_camera=False, rename_with_euler=False,
                           render_size=1024, fps=15, return_frames=False, pbr_model=None, normal_map=None):
        """turntable of a textured mesh on a white background.  mesh_obj: path to a textured .glb, a TexturedMesh
        (renderer_inverse.py) or (verts, faces, uvs01, texture_u8_top_down[, vertex_normals]).
        video_type: 'rgb' or a geometry buffer of the same mesh ('world_normal', 'camera_normal', 'world_position', 'camera_position',
        'z_depth', 'distance'; export_nvdiffrast_video.py:157-175): normals / positions mapped x*0.5+0.5, depths normalised with the (min, max) of
        the FIRST frame's covered pixels (later frames may leave [0, 1] and are clamped in the file).  Vertex normals are
        _vertex_normals(self.normal_weighting) unless the mesh tuple brings its own.
        return_frames: True -> the uint8 frames, 'rgba' -> the float RGBA frames of export_video (geometry types only).
        pbr_model: a pbr.PBRModel -> the 'rgb' frames are lit by its environment (utx_pbr_shade: NVDiffRendererPBR.render_base / render_pbr,
        render/nvdiffrast/renderer_pbr.py:19-94, alpha = coverage) instead of the unlit texture fetch.  map_Ks = (-, roughness, metallic) is the mesh's
        .metallic_roughness (a TexturedMesh of the 9-channel bake; glTF's G / B channels) or a sixth tuple element (uint8, top-down like the texture), else
        the reference's default [1, 1, 0].  None: the unlit path, unchanged.
        normal_map (with pbr_model only): a tangent-space normal map (uint8, top-down like the texture; glTF's normalTexture, OpenGL convention) perturbs the
        shading normal (utx_pbr_shade_nm: bsdf_prepare_shading_normal, two-sided, bent towards the face normal at grazing angles; tangents from
        meshes.vertex_tangents, mirrored UV charts not handled).  True takes the mesh's own map: a TexturedMesh's .bump, a seventh tuple element or, for a
        .glb path, the material's normalTexture; an array is used as the map.  None: the interpolated vertex normal shades, as before."""
        ext = os.path.splitext(video_path)[1]
        assert ext in [".mp4", ".gif"]
        assert video_type in ["rgb", "albedo", "world_normal", "camera_normal", "world_position", "camera_position", "z_depth", "distance"]
        if video_type == "albedo":       # uv_rendering has no render_albedo: the reference's render_result['albedo'] raises (export_video :103)
            raise KeyError("albedo")
        assert return_frames != "rgba" or video_type != "rgb", "return_frames='rgba' is for the geometry video types"
        if pbr_model is not None and video_type != "rgb":
            raise ValueError("pbr_model lights the 'rgb' video only, not video_type=%r" % (video_type,))
        if normal_map is not None and pbr_model is None:
            raise ValueError("normal_map perturbs the shading normal of the lit video: it needs pbr_model")
        vnrm, tex_ks, tex_nm = None, None, None
        if isinstance(mesh_obj, str):
            if normal_map is True and not mesh_obj.lower().endswith(".glb"):
                raise ValueError("normal_map=True reads the normalTexture of a .glb, not of %r" % (mesh_obj,))
            verts, faces, uvs, tex = meshes.load_mesh(mesh_obj)
            verts = meshes.normalise_to_bbox(verts, 1.0)              # texture.mesh.scale_to_bbox() (:178)
            if normal_map is True:
                tex_nm = meshes.load_material_textures(mesh_obj)["normal"]
        elif isinstance(mesh_obj, (tuple, list)):
            verts, faces, uvs, tex = mesh_obj[:4]
            vnrm = mesh_obj[4] if len(mesh_obj) > 4 else None
            tex_ks = mesh_obj[5] if len(mesh_obj) > 5 else None
            tex_nm = mesh_obj[6] if len(mesh_obj) > 6 else None
        else:
            verts, faces, uvs, tex = mesh_obj.vertices, mesh_obj.faces, mesh_obj.uv, mesh_obj.texture
            tex_ks = getattr(mesh_obj, "metallic_roughness", None)
            tex_nm = getattr(mesh_obj, "bump", None)
        if normal_map is True:
            if tex_nm is None:
                raise ValueError("normal_map=True, but the mesh brings no normal map")
        else:
            tex_nm = normal_map
        assert uvs is not None and tex is not None, "missing map_Kd in texture"
        if enhance_mode is None:
            c2ws = camera.generate_orbit_views_c2ws(n_frames + 1, radius=2.8, height=0.0, theta_0=0.0, degree=True)[:n_frames]
        elif enhance_mode == "pitch":
            c2ws = torch.cat([camera.generate_orbit_views_c2ws(n_frames + 1, radius=2.8, height=h, theta_0=0.0, degree=True)[:n_frames]
                              for h in (-2.425, -1.4, 0.0, 1.4, 2.425)])
        elif enhance_mode == "box":
            c2ws = camera.generate_box_views_c2ws(radius=2.8)
        elif enhance_mode == "canonical":
            c2ws = camera.generate_canonical_views_c2ws(radius=2.8, steps=(8, 8, 8))      # 512 frames over the Euler grid (export_nvdiffrast_video.py:204-205)
        else:
            raise NotImplementedError("enhance_mode %s is not supported" % enhance_mode)
        intrinsics = (camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True) if perspective
                      else camera.generate_intrinsics(0.85, 0.85, fov=False, degree=False))
        dev = self.device
        vd = torch.as_tensor(np.asarray(verts), dtype=torch.float32, device=dev).contiguous()
        fd = torch.as_tensor(np.asarray(faces), dtype=torch.int32, device=dev).contiguous()
        uvd = torch.as_tensor(np.asarray(uvs), dtype=torch.float32, device=dev).contiguous()
        # the stored texture image is top-down (row 0 = v = 1); the sampler wants rows growing with v
        # (uint8 -> float on the host: an exact IEEE division, like the reference's image_to_tensor; torch's GPU
        # division by a scalar multiplies by the reciprocal and differs in the last ulp)
        texd = torch.from_numpy(np.ascontiguousarray(np.asarray(tex)[::-1, :, :3]).astype(np.float32) / np.float32(255.0)).to(dev).contiguous()
        mvp = torch.matmul(camera.intr_to_proj(intrinsics, perspective=perspective), camera.c2w_to_w2c(c2ws)).to(dev).contiguous()
        clip, _ = ops.transform_points(vd, mvp, want_ndc=False)
        frames, rgba = [], []
        if pbr_model is not None:
            to_tex = lambda t: torch.from_numpy(np.ascontiguousarray(np.asarray(t)[::-1, :, :3]).astype(np.float32) / np.float32(255.0)).to(dev).contiguous()
            ksd = to_tex(tex_ks) if tex_ks is not None else None
            nd = (torch.as_tensor(np.asarray(vnrm), dtype=torch.float32) if vnrm is not None
                  else _vertex_normals(torch.as_tensor(np.asarray(verts), dtype=torch.float32), torch.as_tensor(np.asarray(faces)), self.normal_weighting))
            nm_args = {}
            if tex_nm is not None:      # tangents (host, fp64) and face normals once per mesh
                nm_args = dict(v_tng=meshes.vertex_tangents(verts, faces, uvs, nd).to(dev).contiguous(), f_nrm=ops.face_normals(vd, fd), normal_map=to_tex(tex_nm))
            nd = nd.to(dev).contiguous()
            for i in range(c2ws.shape[0]):
                rast = ops.rasterize(clip[i].contiguous(), fd, render_size, render_size)
                frames.append(ops.pbr_shade(rast, fd, vd, nd, uvd, texd, ksd, c2ws[i, :3, 3].tolist(), pbr_model.light_diffuse, pbr_model.light_specular,
                                            pbr_model.FG_LUT[0], bg=(1.0, 1.0, 1.0), **nm_args).cpu().numpy())
        elif video_type == "rgb":
            for i in range(c2ws.shape[0]):
                rast = ops.rasterize(clip[i].contiguous(), fd, render_size, render_size)
                frames.append(ops.texture_shade(rast, uvd, fd, texd, bg=(1.0, 1.0, 1.0)).cpu().numpy())
        else:
            # per-view vertex attributes in one launch each for all frames; utx_transform_points has the reference's row layout
            # ([x, y, z, 1] @ M^T), so M = w2c gives the camera-space positions and M = mvp the clip w (no copies: strided views)
            if video_type in ("world_normal", "camera_normal"):
                nd = (torch.as_tensor(np.asarray(vnrm), dtype=torch.float32) if vnrm is not None
                      else _vertex_normals(torch.as_tensor(np.asarray(verts), dtype=torch.float32), torch.as_tensor(np.asarray(faces)), self.normal_weighting))
                nd = nd.to(dev).contiguous()
                per_view = ops.camera_normals(nd, c2ws.to(dev, torch.float32).contiguous()) if video_type == "camera_normal" else None
                attr_of = (lambda i: per_view[i]) if per_view is not None else (lambda i: nd)
            elif video_type == "world_position":
                attr_of = lambda i: vd
            elif video_type == "z_depth":
                attr_of = lambda i: clip[i, :, 3:]
            else:
                cam, _ = ops.transform_points(vd, camera.c2w_to_w2c(c2ws).to(dev, torch.float32).contiguous(), want_ndc=False)
                attr_of = lambda i: cam[i, :, :3]
            normalize, ndc = video_type in ("z_depth", "distance"), video_type not in ("z_depth", "distance")
            scale = None
            for i in range(c2ws.shape[0]):
                rast = ops.rasterize(clip[i].contiguous(), fd, render_size, render_size)
                if normalize and i == 0:      # (min, max) of the first frame's covered pixels, reused by every frame (export_video :120-125)
                    scale = ops.gbuffer_range(video_type, rast, fd, attr_of(0))
                u8 = ops.gbuffer_shade(video_type, rast, fd, attr_of(i), scale2=scale[:2] if normalize else None, ndc=ndc,
                                       bg=(1.0, 1.0, 1.0), want_rgba=return_frames == "rgba")
                if return_frames == "rgba":
                    u8, fl = u8
                    rgba.append(fl.cpu().numpy())
                if normalize and i == 0:      # the flag rides on frame 0's copy: one transfer, no extra synchronisation
                    host = torch.cat([scale.view(torch.uint8), u8.reshape(-1)]).cpu().numpy()
                    if host[8:12].view(np.int32)[0] != 0:
                        raise RuntimeError("video_type %s: the first frame covers no pixel, there is no (min, max) to normalise with" % video_type)
                    frames.append(host[12:].reshape(render_size, render_size, 3))
                else:
                    frames.append(u8.cpu().numpy())
        os.makedirs(os.path.dirname(os.path.abspath(video_path)), exist_ok=True)
        if ext == ".gif":
            write_gif(video_path, frames, fps)
        else:
            write_mjpeg_mp4(video_path, frames, fps)
        base = os.path.splitext(video_path)[0]
        if save_frames:
            os.makedirs(base + "_frames", exist_ok=True)
            for i, fr in enumerate(frames):
                Image.fromarray(fr).save(os.path.join(base + "_frames", "%04d.png" % i))
        if save_cover:
            Image.fromarray(frames[0]).save(base + "_cover.png")
        if save_grid:
            nc = int(math.floor(math.sqrt(len(frames)))); nr = int(math.ceil(len(frames) / nc))
            pad = frames + [np.zeros_like(frames[0])] * (nc * nr - len(frames))
            g = np.stack(pad).reshape(nr, nc, render_size, render_size, 3).transpose(0, 2, 1, 3, 4).reshape(nr * render_size, nc * render_size, 3)
            Image.fromarray(g).save(base + "_grid.png")
        if save_camera:
            torch.save({"c2ws": c2ws, "intrinsics": intrinsics, "perspective": perspective}, base + "_camera.pth")
        if return_frames == "rgba":
            return rgba
        return frames if return_frames else video_path


def write_gif(path, frames, fps=15):
    ims = [Image.fromarray(f) for f in frames]
    ims[0].save(path, save_all=True, append_images=ims[1:], duration=int(round(1000.0 / fps)), loop=0)


def _box(kind, payload):
    return struct.pack(">I4s", 8 + len(payload), kind) + payload


def _full(kind, version, flags, payload):
    return _box(kind, struct.pack(">I", (version << 24) | flags) + payload)


def write_mjpeg_mp4(path, frames, fps=15, quality=92):
    """ISO base media file with one video track of JPEG samples (sample entry 'jpeg', one sample per chunk).
    The image has no H.264 encoder (imageio / ffmpeg are absent); Motion-JPEG plays in ffmpeg, VLC and QuickTime."""
    def enc(f):
        b = io.BytesIO()
        Image.fromarray(f).save(b, format="JPEG", quality=quality)
        return b.getvalue()
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=8) as pool:      # libjpeg releases the GIL: 120 frames of 1024^2 take 0.2 s on one thread
        jpgs = list(pool.map(enc, frames))
    h, w = frames[0].shape[:2]
    n = len(jpgs)
    ftyp = _box(b"ftyp", b"isom" + struct.pack(">I", 512) + b"isomiso2mp41")
    mdat_payload = b"".join(jpgs)
    mdat = _box(b"mdat", mdat_payload)
    first = len(ftyp) + 8
    offsets, pos = [], first
    for j in jpgs:
        offsets.append(pos); pos += len(j)
    ident = struct.pack(">9I", 0x10000, 0, 0, 0, 0x10000, 0, 0, 0, 0x40000000)
    dur_ms = int(round(n * 1000.0 / fps))
    mvhd = _full(b"mvhd", 0, 0, struct.pack(">IIII", 0, 0, 1000, dur_ms) + struct.pack(">IH", 0x10000, 0x100) + b"\x00" * 10 + ident +
                 b"\x00" * 24 + struct.pack(">I", 2))
    tkhd = _full(b"tkhd", 0, 3, struct.pack(">IIIII", 0, 0, 1, 0, dur_ms) + b"\x00" * 8 + struct.pack(">HHHH", 0, 0, 0, 0) + ident +
                 struct.pack(">II", w << 16, h << 16))
    mdhd = _full(b"mdhd", 0, 0, struct.pack(">IIII", 0, 0, int(fps), n) + struct.pack(">HH", 0x55C4, 0))
    hdlr = _full(b"hdlr", 0, 0, struct.pack(">I4s", 0, b"vide") + b"\x00" * 12 + b"unitex_amd turntable\x00")
    vmhd = _full(b"vmhd", 0, 1, b"\x00" * 8)
    dinf = _box(b"dinf", _full(b"dref", 0, 0, struct.pack(">I", 1) + _full(b"url ", 0, 1, b"")))
    entry = (b"\x00" * 6 + struct.pack(">H", 1) + b"\x00" * 16 + struct.pack(">HH", w, h) + struct.pack(">II", 0x480000, 0x480000) +
             struct.pack(">I", 0) + struct.pack(">H", 1) + bytes([10]) + b"Photo-JPEG".ljust(31, b"\x00") + struct.pack(">Hh", 0x18, -1))
    stsd = _full(b"stsd", 0, 0, struct.pack(">I", 1) + _box(b"jpeg", entry))
    stts = _full(b"stts", 0, 0, struct.pack(">III", 1, n, 1))
    stsc = _full(b"stsc", 0, 0, struct.pack(">IIII", 1, 1, 1, 1))
    stsz = _full(b"stsz", 0, 0, struct.pack(">II", 0, n) + b"".join(struct.pack(">I", len(j)) for j in jpgs))
    stco = _full(b"stco", 0, 0, struct.pack(">I", n) + b"".join(struct.pack(">I", o) for o in offsets))
    stbl = _box(b"stbl", stsd + stts + stsc + stsz + stco)
    minf = _box(b"minf", vmhd + dinf + stbl)
    mdia = _box(b"mdia", mdhd + hdlr + minf)
    moov = _box(b"moov", mvhd + _box(b"trak", tkhd + mdia))
    with open(path, "wb") as f:
        f.write(ftyp); f.write(mdat); f.write(moov)


def read_mjpeg_mp4(path):
    """inverse of write_mjpeg_mp4 (used by the tests): returns (fps, [jpeg bytes])."""
    blob = open(path, "rb").read()

    def find(buf, kinds, start=0, end=None):
        end = len(buf) if end is None else end
        pos = start
        while pos < end:
            size, kind = struct.unpack_from(">I4s", buf, pos)
            if kind == kinds[0]:
                if len(kinds) == 1:
                    return pos + 8, pos + size
                hdr = 8 + (8 if kind == b"stsd" else 0)
                return find(buf, kinds[1:], pos + hdr, pos + size)
            pos += size
        raise KeyError(kinds)
    a, _ = find(blob, [b"moov", b"trak", b"mdia", b"mdhd"])
    fps = struct.unpack_from(">I", blob, a + 12)[0]
    a, _ = find(blob, [b"moov", b"trak", b"mdia", b"minf", b"stbl", b"stsz"])
    n = struct.unpack_from(">I", blob, a + 8)[0]
    sizes = struct.unpack_from(">%dI" % n, blob, a + 12)
    a, _ = find(blob, [b"moov", b"trak", b"mdia", b"minf", b"stbl", b"stco"])
    offs = struct.unpack_from(">%dI" % n, blob, a + 8)
    return fps, [blob[o:o + s] for o, s in zip(offs, sizes)]
