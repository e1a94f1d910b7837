#!/usr/bin/env python
"""Generate the PBR shading fixtures under tests/golden/ from the REFERENCE's own Python, through the same seams as make_golden.py (imported from
there, unchanged):

    python tests/golden/make_golden_pbr_shade.py            # writes tests/golden/g15_pbr_shade.npz and g15_fg_lut.npz

  G15   PBRModel.forward (TextureTools/texturetools/texture/pbr/pbr.py:110-130) run on the CPU.  The object is built WITHOUT its __init__ (which needs cv2
        and the CUDA renderutils plugin) and given seeded random light_diffuse / light_specular of 8^2 faces and a seeded 16 x 16 x 2 FG_LUT.
        The lights are uniform in [2, 4): the reference carries its lookup directions in fp32 (two normalisations and a reflection: up to 8 * 2^-24 on wi), and a
        direction error d moves a bilinear lookup on an N^2 face by N / 2 * d * (texel contrast); with N = 8 that is 1.9e-6 * contrast / maximum.  A contrast of at
        most half the maximum keeps the reference's OWN fp32 rounding under the 1e-6 to which the fp64 restatement is held (tests/test_pbr_cpu.py); with lights
        in [0, 4) that rounding alone reached 1.1e-6 at one pixel.
        dr.texture is STUBBED by the fp64 lookups of oracle/pbr_ref.py (the build's own cube rule, include/unitex_hip.h, and clamp-linear for the table),
        rounded to fp32: the fixture pins the reference's arithmetic around the lookups, not nvdiffrast's sampler.
        Inputs: a 32 x 32 image carried by two triangles (four vertices with un-normalised normals, two of them facing away from the eye), interpolated
        and texture-fetched in fp32 in the kernels' operation order (utx_interpolate, utx_texture_shade) from 32^2 Kd / Ks textures whose Ks holds
        metallic 0 and 1 and roughness 0 and 1.  Stored: the mesh-level inputs (rast, faces, vertices, textures), the dense inputs the reference saw, the
        three lookup coordinate sets and results, and the reference's diffuse / specular.
  g15_fg_lut.npz: the reference's envmaps/bsdf_256_256.bin as float32 [256][256][2] (data its PBRModel reads; used by the tests only)."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import REF, install_stubs  # noqa: E402
from oracle.pixel_ref import interp  # noqa: E402

F32 = np.float32
S = 32


def _fetch(tex, uv):
    """utx_texture_shade's fetch in fp32: bilinear, wrap, t00 (1 - fx) + t01 fx"""
    Ht, Wt = tex.shape[:2]
    x, y = uv[..., 0] * F32(Wt) - F32(0.5), uv[..., 1] * F32(Ht) - F32(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    ix = lambda t: np.mod(t.astype(np.int64), Wt)
    iy = lambda t: np.mod(t.astype(np.int64), Ht)
    one = F32(1.0)
    top = tex[iy(y0), ix(x0)] * (one - fx) + tex[iy(y0), ix(x0 + 1)] * fx
    bot = tex[iy(y0 + 1), ix(x0)] * (one - fx) + tex[iy(y0 + 1), ix(x0 + 1)] * fx
    return (top * (one - fy) + bot * fy).astype(F32)


def g15(out):
    from oracle import pbr_ref as PC
    P = importlib.import_module("TextureTools.texturetools.texture.pbr.pbr")
    dr = importlib.import_module("nvdiffrast.torch")
    rng = np.random.default_rng(15)
    light_d = rng.uniform(2.0, 4.0, (6, 8, 8, 3)).astype(F32)
    light_s = rng.uniform(2.0, 4.0, (6, 8, 8, 3)).astype(F32)
    lut = rng.uniform(0.0, 1.0, (16, 16, 2)).astype(F32)
    # the quad: two triangles over the 32 x 32 image, pixel centres strictly inside; (u, v) = weights of vertices 0 and 1
    verts = np.array([[-0.9, -0.7, 0.2], [0.8, -0.8, -0.3], [0.9, 0.7, 0.4], [-0.7, 0.9, -0.2]], F32)
    nrm = np.array([[0.3, 0.2, 1.9], [-0.4, 0.1, 0.6], [0.5, -0.9, -0.4], [-0.2, 0.8, -1.3]], F32)      # lengths 0.7 .. 1.9; vertices 2, 3 face away
    uvs = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], F32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    eye = np.array([0.4, -0.6, 2.8], F32)
    g = ((np.arange(S) + 0.5) / S).astype(F32)
    yy, xx = np.meshgrid(g, g, indexing="ij")
    rast = np.zeros((S, S, 4), F32)
    lower = xx >= yy                      # triangle 0 = (0, 1, 2): weights (1 - x, x - y, y); triangle 1 = (0, 2, 3): weights (1 - y, x, y - x)
    rast[..., 0] = np.where(lower, F32(1.0) - xx, F32(1.0) - yy)
    rast[..., 1] = np.where(lower, xx - yy, xx)
    rast[..., 2] = 0.5
    rast[..., 3] = np.where(lower, 1.0, 2.0)
    kd = rng.uniform(0.0, 1.0, (S, S, 3)).astype(F32)
    ks = rng.uniform(0.0, 1.0, (S, S, 3)).astype(F32)
    ks[:8, :, 2], ks[8:16, :, 2] = 0.0, 1.0          # metallic 0 and 1
    ks[:, :8, 1], ks[:, 8:16, 1] = 0.0, 1.0          # roughness 0 and 1
    pos_i, nrm_i, uv_i = (interp(a, rast, faces)[0] for a in (verts, nrm, uvs))
    kd_i, ks_i = _fetch(kd, uv_i), _fetch(ks, uv_i)
    log = {}

    def texture(tex, uv, filter_mode="linear", boundary_mode="wrap", **kw):
        assert filter_mode == "linear"
        t, c = tex[0].numpy(), uv.numpy()
        if boundary_mode == "cube":
            r = PC.cube_lookup(t, c)
            key = "diffuse" if "diffuse_coord" not in log else "specular"
        else:
            assert boundary_mode == "clamp"
            r = PC.lut_lookup(t, c)
            key = "fg"
        log[key + "_coord"], log[key + "_lookup"] = c.astype(F32), r.astype(F32)
        return torch.from_numpy(r.astype(F32))
    dr.texture = texture
    model = P.PBRModel.__new__(P.PBRModel)
    torch.nn.Module.__init__(model)
    model.light_diffuse, model.light_specular, model.FG_LUT = torch.from_numpy(light_d), torch.from_numpy(light_s), torch.from_numpy(lut)[None]
    t = torch.from_numpy
    diffuse, specular = model.forward(t(eye).reshape(1, 1, 1, 3), t(pos_i)[None], t(nrm_i)[None], t(kd_i)[None], t(ks_i)[None])
    fix = dict(light_diffuse=light_d, light_specular=light_s, fg_lut=lut, verts=verts, v_nrm=nrm, uvs=uvs, faces=faces, rast=rast, tex_Kd=kd, tex_Ks=ks,
               view_position=eye, world_position=pos_i, world_normal=nrm_i, map_Kd=kd_i, map_Ks=ks_i, diffuse=diffuse[0].numpy(), specular=specular[0].numpy())
    for k, v in log.items():
        fix[k] = v[0]
    assert fix["diffuse"].shape == (S, S, 3) and np.isfinite(fix["diffuse"]).all() and np.isfinite(fix["specular"]).all()
    path = os.path.join(out, "g15_pbr_shade.npz")
    np.savez_compressed(path, **fix)
    print("G15: %d arrays, %d bytes" % (len(fix), os.path.getsize(path)))


def fg_lut(out):
    raw = np.fromfile(os.path.join(REF, "TextureTools", "texturetools", "texture", "pbr", "envmaps", "bsdf_256_256.bin"), dtype=np.float32)
    path = os.path.join(out, "g15_fg_lut.npz")
    np.savez_compressed(path, fg_lut=raw.reshape(256, 256, 2))
    print("g15_fg_lut: %d bytes" % os.path.getsize(path))


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g15(out)
    fg_lut(out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
