"""Image-based PBR shading: the environment light of the reference's PBRModel (TextureTools/texturetools/texture/pbr/pbr.py:18-49, 91-130) and
its two prefilters (texture/pbr/renderutils/ops.py:398-465), on the HIP kernels of csrc/pbr.hip.

    model = PBRModel("studio.hdr", device="cuda:0")          # lat-long map -> cubemap -> diffuse / specular light, split-sum table
    VideoExporter().export_orbit_video(mesh, "turntable.mp4", pbr_model=model)

Colour order: the reference reads its map with cv2.imread and hands the BGR array to the shader as it is; here the map stays RGB (read_hdr and PIL both
return RGB), which is what the file means.
Tangent-space normal maps (the bump texture of the 9-channel bake, glTF's normalTexture): export_orbit_video(normal_map=...) shades with
bsdf_prepare_shading_normal's normal (renderutils/bsdf.py:28-51, two-sided, OpenGL convention; ops.pbr_shading_normal, ops.pbr_shade(normal_map=...));
mirrored UV charts (tangent handedness -1) are not handled, as in the reference.
Not built (the reference's render_pbr has them or nvdiffrast does): dr.antialias (ops.antialias exists, it is not wired here), backward passes, and render_pbr's lambda_* knobs other than
lambda_diffuse / lambda_specular."""
import re

import numpy as np
import torch


def read_hdr(path):
    """Radiance RGBE (.hdr) -> float32 [H,W,3] RGB, rows top-down.  Flat and new-RLE scanlines, '-Y h +X w' orientation only."""
    blob = open(path, "rb").read()
    if not (blob.startswith(b"#?RADIANCE") or blob.startswith(b"#?RGBE")):
        raise ValueError("%s: not a Radiance RGBE file" % path)
    end = blob.find(b"\n\n")
    if end < 0:
        raise ValueError("%s: header without end" % path)
    if b"FORMAT=32-bit_rle_rgbe" not in blob[:end]:
        raise ValueError("%s: only FORMAT=32-bit_rle_rgbe is read" % path)
    eol = blob.find(b"\n", end + 2)
    m = re.match(rb"-Y (\d+) \+X (\d+)$", blob[end + 2:eol].strip())
    if not m:
        raise ValueError("%s: only the '-Y h +X w' orientation is read" % path)
    h, w = int(m.group(1)), int(m.group(2))
    data = np.frombuffer(blob, np.uint8, offset=eol + 1)
    rgbe = np.empty((h, w, 4), np.uint8)
    pos = 0
    for y in range(h):
        if 8 <= w < 32768 and data[pos] == 2 and data[pos + 1] == 2 and (int(data[pos + 2]) << 8 | int(data[pos + 3])) == w:
            pos += 4
            for c in range(4):          # new RLE: the four components of the scanline one after the other
                x = 0
                while x < w:
                    n = int(data[pos])
                    if n > 128:
                        n -= 128
                        if x + n > w:
                            raise ValueError("%s: run past the end of scanline %d" % (path, y))
                        rgbe[y, x:x + n, c] = data[pos + 1]
                        pos += 2
                    else:
                        if n == 0 or x + n > w:
                            raise ValueError("%s: bad literal count in scanline %d" % (path, y))
                        rgbe[y, x:x + n, c] = data[pos + 1:pos + 1 + n]
                        pos += 1 + n
                    x += n
        else:
            rgbe[y] = data[pos:pos + 4 * w].reshape(w, 4)
            pos += 4 * w
    e = rgbe[..., 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)          # mantissa / 256 * 2^(e - 128)
    return (rgbe[..., :3].astype(np.float64) * scale[..., None]).astype(np.float32)


def read_env(path):
    """environment map file -> float32 [H,W,3] RGB: .hdr through read_hdr, everything else through PIL (uint8 images as / 255, pbr.py:100-102)"""
    if path.lower().endswith(".hdr"):
        return read_hdr(path)
    from PIL import Image
    a = np.asarray(Image.open(path).convert("RGB"))
    return (a.astype(np.float32) / np.float32(255.0)) if a.dtype == np.uint8 else a.astype(np.float32)


def ndf_cutoff(roughness, cutoff, n_samples=1000000):
    """cosine of the angle inside which the GGX lobe of `roughness` holds `cutoff` of its mass: __ndfBounds' search (renderutils/ops.py:435-445), numpy fp64"""
    a2 = float(roughness) ** 4
    costheta = np.cos(np.linspace(0, np.pi / 2.0, n_samples))
    c = np.clip(costheta, 0.0, 1.0)
    d = (c * a2 - c) * c + 1.0
    D = np.cumsum(a2 / (d * d * np.pi))
    return float(costheta[np.argmax(D >= D[..., -1] * cutoff)])


def latlong_to_cubemap(latlong, res):
    """latlong [Hi,Wi,3] (CUDA float32 tensor) -> cubemap [6,res,res,3] (pbr.py:28-49; res: int or [res, res])"""
    from . import ops
    if not isinstance(res, int):
        assert res[0] == res[1], "square faces only"
        res = int(res[0])
    return ops.latlong_to_cubemap(latlong.contiguous(), res)


class PBRModel:
    """The reference's PBRModel on HIP kernels.  env: None (the reference's default, a 4x4x3 map of ones), a path (.hdr or an image) or an [H,W,3] array / tensor.
    light_diffuse / light_specular: [6,cube_res,cube_res,3]; FG_LUT: [1,R,R,2] (fg_lut=None: utx_dfg_lut at 256^2, 1024 samples; an array is used as given)."""

    def __init__(self, env=None, device="cuda", cube_res=512, roughness=0.08, cutoff=0.99, fg_lut=None):
        from . import ops
        self.device = torch.device(device if device != "cuda" else "cuda:%d" % torch.cuda.current_device())
        if env is None:
            latlong = np.ones((4, 4, 3), np.float32)
        elif isinstance(env, str):
            latlong = read_env(env)
        else:
            latlong = env
        latlong = torch.as_tensor(np.asarray(latlong.cpu() if torch.is_tensor(latlong) else latlong), dtype=torch.float32)
        assert latlong.dim() == 3 and latlong.shape[-1] == 3, "environment map must be [H,W,3]"
        with torch.cuda.device(self.device):
            if fg_lut is None:
                lut = ops.dfg_lut(256, 1024, self.device)
            else:
                lut = torch.as_tensor(np.asarray(fg_lut.cpu() if torch.is_tensor(fg_lut) else fg_lut), dtype=torch.float32).to(self.device)
                lut = lut.reshape(lut.shape[-3], lut.shape[-2], 2).contiguous()
                assert lut.shape[0] == lut.shape[1], "FG_LUT must be square"
            self.FG_LUT = lut.unsqueeze(0)
            self.costheta_cutoff = ndf_cutoff(roughness, cutoff)
            cubemap = ops.latlong_to_cubemap(latlong.to(self.device).contiguous(), int(cube_res))
            texels, tiles = ops.cubemap_tables(int(cube_res), self.costheta_cutoff, self.device)
            self.light_diffuse = ops.cubemap_diffuse(cubemap, texels)
            self.light_specular = ops.cubemap_specular(cubemap, roughness, self.costheta_cutoff, texels, tiles)

    def forward(self, view_position, world_position, world_normal, map_Kd, map_Ks):
        """pbr.py:110-130 on dense tensors [..., 3] (map_Kd may carry an alpha channel; view_position broadcasts) -> (diffuse, specular) [..., 3]"""
        from . import ops
        shape = world_position.shape
        f = lambda t, c: t.to(self.device, torch.float32).expand(shape[:-1] + (c,)).reshape(-1, c).contiguous()
        view = view_position.to(self.device, torch.float32)
        view = view.reshape(3).contiguous() if view.numel() == 3 else f(view, 3)
        d, s = ops.pbr_forward(view, f(world_position, 3), f(world_normal, 3), f(map_Kd, map_Kd.shape[-1]), f(map_Ks, 3), self.light_diffuse,
                               self.light_specular, self.FG_LUT[0])
        return d.reshape(shape), s.reshape(shape)

    __call__ = forward
