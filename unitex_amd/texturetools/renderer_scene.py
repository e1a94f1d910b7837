"""Geometry renderer for panoramas and cubemaps: the call surface of the reference's NVDiffRendererScene
(TextureTools/texturetools/render/nvdiffrast/renderer_scene.py) over the HIP kernels of csrc/scene.hip.

  layout      grid_to_cube, cubemap_to_flatten, cubemap_to_flatten_kjl, flatten_to_cubemap: slicing and flips on the device, no kernel
  conversion  latlong_to_cubemap (the existing utx_latlong_to_cubemap), cubemap_to_latlong (utx_cubemap_to_latlong), latlong_depth_to_pcd (elementwise)
  the class   perspective_rendering (utx_scene_render), perspective_inverse_rendering_torch (utx_scene_render + utx_scene_bake_latlong)

A cubemap is read by this library's own cube lookup rule (include/unitex_hip.h), not by nvdiffrast's boundary_mode='cube' sampler.

Kept from the reference, on purpose:
  * render_latlong_map without render_uv returns no map: the branch is nested under render_uv there (:308-316, :401-429);
  * perspective_inverse_rendering_torch is written for ONE shared [3, 3] intrinsics matrix (its own broadcast fails for [M, 3, 3]); [M, 3, 3] is accepted here
    in addition; perspective_rendering takes either, as the reference does;
  * the bake projects the panorama's unit direction as a POINT (rd, 1), so a camera's translation moves its footprint;
  * cubemap_to_latlong and latlong_to_cubemap are not inverses of each other.
Refused, never silently dropped: render_cubemap=True in the inverse renderer (NotImplementedError, as the reference's own branch), the scipy interpolator
(NotImplementedError: a host-side Delaunay LinearNDInterpolator), a requested lookup whose map is None (ValueError), unknown keywords (TypeError)."""
import numpy as np
import torch

from . import camera, ops
from .pbr import latlong_to_cubemap  # noqa: F401  (re-export: the reference keeps it in this module)

__all__ = ["grid_to_cube", "cubemap_to_flatten", "cubemap_to_flatten_kjl", "flatten_to_cubemap", "latlong_to_cubemap", "cubemap_to_latlong",
           "latlong_depth_to_pcd", "image_to_tensor", "NVDiffRendererScene"]


def _hw(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


# ---------------------------------------------------------------------------------------------------------------- layout
def grid_to_cube(x, y):
    """x, y [H,W] -> [6,H,W,3]: faces right, left, top, down, back, front = (1,-y,-x) (-1,-y,x) (x,1,y) (x,-1,-y) (x,-y,1) (-x,-y,-1)"""
    x, y = torch.broadcast_tensors(x, y)
    one = torch.ones_like(x)
    faces = [(one, -y, -x), (-one, -y, x), (x, one, y), (x, -one, -y), (x, -y, one), (-x, -y, -one)]
    return torch.stack([torch.stack(f, dim=-1) for f in faces], dim=0)


# the cross:      top              each entry: (face, block row, block column, flips)
#           left front right back
#                 down
_CROSS = [(2, 0, 1, (0,)), (1, 1, 0, (1,)), (5, 1, 1, (1,)), (0, 1, 2, (1,)), (4, 1, 3, (1,)), (3, 2, 1, (0,))]


def cubemap_to_flatten(cubemap):
    """[6,H,W,C] (right, left, top, down, back, front) -> the flattened cross [3H,4W,C], zeros elsewhere"""
    _, H, W, C = cubemap.shape
    flat = torch.zeros((3 * H, 4 * W, C), dtype=cubemap.dtype, device=cubemap.device)
    for s, r, c, flips in _CROSS:
        flat[r * H:(r + 1) * H, c * W:(c + 1) * W] = cubemap[s].flip(flips)
    return flat


def flatten_to_cubemap(flatten):
    """the inverse of cubemap_to_flatten: [3H,4W,C] -> [6,H,W,C]"""
    HF, WF, C = flatten.shape
    H, W = HF // 3, WF // 4
    cube = torch.zeros((6, H, W, C), dtype=flatten.dtype, device=flatten.device)
    for s, r, c, flips in _CROSS:
        cube[s] = flatten[r * H:(r + 1) * H, c * W:(c + 1) * W].flip(flips)
    return cube


def cubemap_to_flatten_kjl(cubemap):
    """the kujiale dataset's face order into the same cross: faces 1-4 along the middle row as they are, face 0 on top and face 5 below, both turned"""
    _, H, W, C = cubemap.shape
    flat = torch.zeros((3 * H, 4 * W, C), dtype=cubemap.dtype, device=cubemap.device)
    flat[:H, W:2 * W] = cubemap[0].transpose(0, 1).flip(1)
    for k in range(4):
        flat[H:2 * H, k * W:(k + 1) * W] = cubemap[1 + k]
    flat[2 * H:, W:2 * W] = cubemap[5].transpose(0, 1).flip(0)
    return flat


# ---------------------------------------------------------------------------------------------------------------- conversion
def cubemap_to_latlong(cubemap, render_size):
    """cubemap [6,N,N,C] -> panorama [Ho,Wo,C] (utx_cubemap_to_latlong).  Not the inverse of latlong_to_cubemap."""
    Ho, Wo = _hw(render_size)
    return ops.cubemap_to_latlong(cubemap.to(dtype=torch.float32).contiguous(), Ho, Wo)


def _latlong_dirs(H, W, dtype, device):
    gy, gx = torch.meshgrid(torch.linspace(-1.0 + 1.0 / H, 1.0 - 1.0 / H, H, dtype=dtype, device=device),
                            torch.linspace(-1.0 + 1.0 / W, 1.0 - 1.0 / W, W, dtype=dtype, device=device), indexing="ij")
    psi, theta = gx * torch.pi, gy * (torch.pi / 2) + torch.pi / 2
    return torch.stack([torch.sin(theta) * torch.sin(psi), torch.cos(theta), -torch.sin(theta) * torch.cos(psi)], dim=-1)


def latlong_depth_to_pcd(depth):
    """depth [H,W,1] -> xyz [H,W,3] = depth * the panorama's direction grid"""
    H, W, _ = depth.shape
    return depth * _latlong_dirs(H, W, depth.dtype, depth.device)


_MODE_MAX = {"I": 4294967295.0, "I;16": 65535.0, "I;16B": 65535.0, "F": 1.0}


def image_to_tensor(image, device="cuda"):
    """a PIL image [H,W,3] or a list of them [n,H,W,3], float32 in [0, 1]: grey is repeated to RGB, two channels get a third of ones, an alpha is cut off
    (the division runs on the host: an exact IEEE division)"""
    many = isinstance(image, (list, tuple))
    ims = list(image) if many else [image]
    a = np.stack([np.array(im, dtype=np.float32) for im in ims], axis=0) / np.float32(_MODE_MAX.get(ims[0].mode, 255.0))
    if a.ndim == 3:
        a = a[..., None]
    if a.ndim != 4:
        raise NotImplementedError("image.ndim %d is not supported" % (a.ndim - 1))
    if a.shape[-1] == 1:
        a = np.tile(a, (1, 1, 1, 3))
    elif a.shape[-1] == 2:
        a = np.concatenate([a, np.ones_like(a[..., :1])], axis=-1)
    a = np.ascontiguousarray(a[..., :3])
    return torch.as_tensor(a if many else a[0], dtype=torch.float32, device=device)


# ---------------------------------------------------------------------------------------------------------------- the class
class NVDiffRendererScene:
    def __init__(self, device="cuda", latlong_map=None, cubemap=None):
        self.device = torch.device(device)
        put = lambda t: t.to(device=self.device, dtype=torch.float32).contiguous() if t is not None else None
        self.latlong_map, self.cubemap = put(latlong_map), put(cubemap)
        self.enable_nvdiffrast_cuda_ctx()

    def enable_nvdiffrast_cuda_ctx(self):
        """no rasteriser context is needed here; kept for the call surface"""
        self.ctx = None

    def enable_nvdiffrast_opengl_ctx(self):
        self.ctx = None

    def clear(self):
        self.latlong_map = None
        self.cubemap = None

    @staticmethod
    def _load(device, latlong_map, cubemaps, cubemap_kjl):
        assert latlong_map is not None or cubemaps is not None
        lat = image_to_tensor(latlong_map, device=device) if latlong_map is not None else None
        cube = None
        if cubemaps is not None:
            assert len(cubemaps) == 6
            cube = image_to_tensor(list(cubemaps), device=device)
            if cubemap_kjl:
                cube = flatten_to_cubemap(cubemap_to_flatten_kjl(cube))
        return lat, cube

    @staticmethod
    def _open(latlong_map_path, cubemap_paths):
        from PIL import Image
        return (Image.open(latlong_map_path) if latlong_map_path is not None else None,
                [Image.open(p) for p in cubemap_paths] if cubemap_paths is not None else None)

    @classmethod
    def from_images(cls, device="cuda", latlong_map=None, cubemaps=None, cubemap_kjl=False):
        lat, cube = cls._load(device, latlong_map, cubemaps, cubemap_kjl)
        return cls(device=device, latlong_map=lat, cubemap=cube)

    @classmethod
    def from_files(cls, device="cuda", latlong_map_path=None, cubemap_paths=None, cubemap_kjl=False):
        assert latlong_map_path is not None or cubemap_paths is not None
        return cls.from_images(device, *cls._open(latlong_map_path, cubemap_paths), cubemap_kjl=cubemap_kjl)

    def update_from_images(self, latlong_map=None, cubemaps=None, cubemap_kjl=False):
        lat, cube = self._load(self.device, latlong_map, cubemaps, cubemap_kjl)
        put = lambda t: t.contiguous() if t is not None else None
        self.latlong_map, self.cubemap = put(lat), put(cube)
        return self

    def update_from_files(self, latlong_map_path=None, cubemap_paths=None, cubemap_kjl=False):
        assert latlong_map_path is not None or cubemap_paths is not None
        return self.update_from_images(*self._open(latlong_map_path, cubemap_paths), cubemap_kjl=cubemap_kjl)

    # ---- rendering
    def _cameras(self, c2ws, intrinsics):
        c2ws = c2ws.to(device=self.device, dtype=torch.float32).contiguous()
        intrinsics = intrinsics.to(device=self.device, dtype=torch.float32).contiguous()
        if c2ws.ndim != 3 or c2ws.shape[1:] != (4, 4) or intrinsics.shape not in ((3, 3), (c2ws.shape[0], 3, 3)):
            raise ValueError("c2ws must be [M,4,4] and intrinsics [3,3] or [M,3,3], got %s and %s" % (tuple(c2ws.shape), tuple(intrinsics.shape)))
        return c2ws, intrinsics

    def _rays(self, c2ws, intrinsics, height, width, want, cubemap=None, latlong=None):
        out = {"rays_o": c2ws[:, None, None, :3, 3].expand(-1, height, width, -1)}      # the eye, broadcast as the reference's expand_as does
        out.update(ops.scene_render(c2ws, intrinsics, height, width, cubemap=cubemap, latlong=latlong, want=want))
        return out

    def perspective_rendering(self, c2ws, intrinsics, render_size, render_cubemap=False, render_uv=False, render_latlong_map=False):
        """c2ws [M,4,4], intrinsics [3,3] or [M,3,3] (normalised) -> {'rays_o', 'rays_d' [M,H,W,3]} and, as requested, 'cubemap_attr' [M,H,W,C], 'uv' [M,H,W,2],
        'latlong_map_attr' [M,H,W,C] (only together with render_uv: module docstring).  One launch for every requested output."""
        c2ws, intrinsics = self._cameras(c2ws, intrinsics)
        height, width = _hw(render_size)
        want = ["rays_d"]
        if render_cubemap:
            if self.cubemap is None:
                raise ValueError("render_cubemap needs a cubemap, the renderer holds none")
            want.append("cubemap_attr")
        if render_uv:
            want.append("uv")
            if render_latlong_map:
                if self.latlong_map is None:
                    raise ValueError("render_latlong_map needs a lat-long map, the renderer holds none")
                want.append("latlong_map_attr")
        return self._rays(c2ws, intrinsics, height, width, tuple(want), cubemap=self.cubemap if render_cubemap else None,
                          latlong=self.latlong_map if "latlong_map_attr" in want else None)

    def perspective_inverse_rendering_scipy(self, *args, **kwargs):
        raise NotImplementedError("perspective_inverse_rendering_scipy is scipy's Delaunay LinearNDInterpolator on the host; use perspective_inverse_rendering_torch")

    def perspective_inverse_rendering_torch(self, c2ws, intrinsics, images, render_size, texture_size, render_cubemap=False, render_uv=False,
                                            render_latlong_map=False):
        """c2ws [M,4,4], intrinsics [3,3] (or [M,3,3]), images [M,H,W,C] -> {'rays_o', 'rays_d'} at render_size and, with render_uv, 'uv' [M,Ht,Wt,2] (each
        view's NDC of every panorama texel) and 'uv_alpha' [M,Ht,Wt,1]; with render_latlong_map too, 'latlong_map_attr' [Ht,Wt,C]: the mean of the views that see
        the texel, 0 where none does, clamped to [0, 1]."""
        if render_cubemap:
            raise NotImplementedError("render_cubemap is not implemented in the inverse renderer (nor in the reference)")
        c2ws, intrinsics = self._cameras(c2ws, intrinsics)
        height, width = _hw(render_size)
        height_t, width_t = _hw(texture_size)
        if render_uv and render_latlong_map and images is None:
            raise ValueError("render_latlong_map needs the views' images")
        out = self._rays(c2ws, intrinsics, height, width, ("rays_d",))
        if render_uv:
            # the reference's two matrices, each rounded to fp32 on its own: inverse(c2w) (torch.linalg.inv, on the host: M 4 x 4 matrices) and intr_to_proj
            w2cs = torch.linalg.inv(c2ws.cpu()).to(self.device).contiguous()
            projs = camera.intr_to_proj(intrinsics, perspective=True).expand(c2ws.shape[0], 4, 4).contiguous()
            imgs = None
            if render_latlong_map:
                imgs = images.to(device=self.device, dtype=torch.float32).contiguous()
            uv, alpha, attr = ops.scene_bake_latlong(w2cs, projs, height_t, width_t, imgs)
            out.update({"uv": uv, "uv_alpha": alpha})
            if attr is not None:
                out["latlong_map_attr"] = attr
        return out

