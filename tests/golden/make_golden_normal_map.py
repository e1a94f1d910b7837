#!/usr/bin/env python
"""Generate the normal-map fixture under tests/golden/ from the REFERENCE's own Python, through the same seams as make_golden.py (imported from there,
unchanged):

    python tests/golden/make_golden_normal_map.py            # writes tests/golden/g16_normal_map.npz

  G16   bsdf_prepare_shading_normal(..., two_sided_shading=True, opengl=True) (TextureTools/texturetools/texture/pbr/renderutils/bsdf.py:28-51, plain torch) run
        on the CPU, its result fed to PBRModel.forward (texture/pbr/pbr.py:110-130) exactly as G15 does: the object built without its __init__, seeded lights
        of 8^2 faces uniform in [2, 4) (the contrast bound of make_golden_pbr_shade.py's header: the reference's own fp32 rounding of a lookup direction moves
        a bilinear lookup by N / 2 * d * contrast) and a seeded 16 x 16 x 2 FG_LUT; dr.texture STUBBED by the fp64 lookups of oracle/pbr_ref.py.
        Inputs: a 32 x 32 image carried by four triangles around a centre vertex (five vertices).  Triangle 3 is wound the other way, so its geometric normal
        faces away from the eye (the two-sided flip).  Vertex normals and tangents are un-normalised and not orthogonal; vertex 3's tangent is parallel to its
        normal.  The barycentrics, the uvs and so the texel coordinates (0.75 i + 3) are dyadic: every fourth pixel fetches one texel exactly, the others blend
        with fractions 0.25 / 0.5 / 0.75.  The 32^2 normal-map texture has rows 3..7 of (0.5, 0.5, 1) (the flat map), rows 20..27 with z < 0.5 (negative after
        decode), ONE texel (12, 12) of (0.5, 0.5, 0.5) that pixel (12, 12) fetches exactly (a zero perturbation), and random texels elsewhere, which put many
        pixels into the bend region 0 < dot(vv, s) < 0.1.  Columns 30, 31 of the raster are empty (the background of the fused frame); the dense inputs cover
        all 32 x 32 pixels.  Interpolation and fetches are fp32 in the kernels' operation order.
        Asserted here: min |dot(geom_nrm, vv)| >= 1e-3 over all pixels, so that fp32 and fp64 decide the flip alike and the tests leave out no pixel.
        Stored: the mesh-level inputs (rast, faces, vertices, normals, tangents, face normals, uvs, the three textures), the dense inputs the reference saw, the
        reference's shading normal, diffuse and specular."""
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
from make_golden_pbr_shade import _fetch  # noqa: E402
from oracle.pixel_ref import interp  # noqa: E402

F32 = np.float32
S = 32


def g16(out):
    from oracle import pbr_ref as PC
    P = importlib.import_module("TextureTools.texturetools.texture.pbr.pbr")
    B = importlib.import_module("TextureTools.texturetools.texture.pbr.renderutils.bsdf")
    dr = importlib.import_module("nvdiffrast.torch")
    rng = np.random.default_rng(16)
    light_d = rng.uniform(2.0, 4.0, (6, 8, 8, 3)).astype(F32)
    light_s = rng.uniform(2.0, 4.0, (6, 8, 8, 3)).astype(F32)
    lut = rng.uniform(0.0, 1.0, (16, 16, 2)).astype(F32)
    verts = np.array([[-0.9, -0.7, 0.2], [0.8, -0.8, -0.3], [0.9, 0.7, 0.4], [-0.7, 0.9, -0.2], [0.05, 0.0, 0.35]], F32)
    nrm = np.array([[0.3, 0.2, 1.9], [-0.4, 0.1, 0.6], [0.5, -0.3, 0.7], [-0.2, 0.8, 1.3], [0.1, -0.2, 1.1]], F32)
    tng = np.array([[1.2, 0.1, 0.3], [0.7, 0.2, -0.1], [0.9, -0.4, 0.2], [-0.1, 0.4, 0.65], [1.5, 0.3, -0.4]], F32)      # vertex 3: 0.5 x its normal
    assert np.array_equal(tng[3] * F32(2.0), nrm[3])
    off, span = F32(25.0 / 256.0), F32(0.75)
    uvs = (np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5, 0.5]], F32) * span + off).astype(F32)
    faces = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [0, 3, 4]], np.int32)          # 0..2 counter-clockwise seen from +z, 3 clockwise
    eye = np.array([0.4, -0.6, 2.8], F32)
    g = ((np.arange(S) + 0.5) / S).astype(F32)
    yy, xx = np.meshgrid(g, g, indexing="ij")
    one = F32(1.0)
    # (u, v) = weights of the face's first two vertices; the third (the centre) takes the rest.  All dyadic, exact in fp32.
    bottom, right, top = (yy <= xx) & (yy <= one - xx), (xx > yy) & (xx > one - yy), (yy >= xx) & (yy >= one - xx)
    fid = np.where(bottom, 0, np.where(right, 1, np.where(top, 2, 3)))
    u = np.choose(fid, [one - xx - yy, xx - yy, xx + yy - one, one - xx - yy])
    v = np.choose(fid, [xx - yy, xx + yy - one, yy - xx, yy - xx])
    full = np.zeros((S, S, 4), F32)
    full[..., 0], full[..., 1], full[..., 2], full[..., 3] = u, v, 0.5, fid + 1
    w = (one - full[..., 0]) - full[..., 1]
    assert (full[..., 0] >= 0).all() and (full[..., 1] >= 0).all() and (w >= 0).all()
    corner = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [0.5, 0.5]])
    f = faces[fid]
    back = corner[f[..., 0]] * u[..., None] + corner[f[..., 1]] * v[..., None] + corner[f[..., 2]] * w[..., None]
    assert np.array_equal(back[..., 0], xx) and np.array_equal(back[..., 1], yy), "the barycentrics reproduce the pixel centres exactly"
    kd = rng.uniform(0.0, 1.0, (S, S, 3)).astype(F32)
    ks = rng.uniform(0.0, 1.0, (S, S, 3)).astype(F32)
    nm = rng.uniform(0.0, 1.0, (S, S, 3)).astype(F32)
    nm[3:8] = np.array([0.5, 0.5, 1.0], F32)
    nm[20:28, :, 2] *= F32(0.5)
    nm[12, 12] = 0.5
    fn = np.cross(verts[faces[:, 1]].astype(np.float64) - verts[faces[:, 0]], verts[faces[:, 2]].astype(np.float64) - verts[faces[:, 0]])
    fn = (fn / np.linalg.norm(fn, axis=-1, keepdims=True)).astype(F32)
    pos_i, nrm_i, tng_i, uv_i = (interp(a, full, faces)[0] for a in (verts, nrm, tng, uvs))
    assert np.array_equal(uv_i[..., 0] * F32(S) - F32(0.5), F32(0.75) * np.arange(S, dtype=F32)[None, :] + F32(3.0) + 0 * yy), "texel coordinates 0.75 i + 3"
    kd_i, ks_i, nm_i = _fetch(kd, uv_i), _fetch(ks, uv_i), _fetch(nm, uv_i)
    pert = (F32(2.0) * nm_i - F32(1.0)).astype(F32)
    geom = fn[fid]
    assert (pert[12, 12] == 0).all() and (pert[:, :, 2] < 0).any() and (pert[0, 0] == np.array([0, 0, 1], F32)).all()
    vv = eye.astype(np.float64) - pos_i
    vv /= np.linalg.norm(vv, axis=-1, keepdims=True)
    gd = (geom.astype(np.float64) * vv).sum(-1)
    print("G16: min |dot(geom_nrm, vv)| = %.4g; back-facing pixels %d" % (np.abs(gd).min(), (gd < 0).sum()))
    assert np.abs(gd).min() >= 1e-3
    assert (gd[fid == 3] < 0).all() and (gd[fid != 3] > 0).all()
    t = torch.from_numpy
    sn = B.bsdf_prepare_shading_normal(t(pos_i), t(eye).reshape(1, 1, 3), t(pert), t(nrm_i), t(tng_i), t(geom), two_sided_shading=True, opengl=True)
    assert sn.dtype == torch.float32 and torch.isfinite(sn).all()
    # the bend region, judged on the reference's own result: out = g + t (s - g) with 0 < t < 1 is neither g nor s
    s_ref = B._perturb_normal(t(pert), B._safe_normalize(t(nrm_i)), B._safe_normalize(t(tng_i)), True).numpy().astype(np.float64)
    s_ref = np.where(gd[..., None] > 0, s_ref, -s_ref)
    vs = (vv * s_ref).sum(-1)
    bend = (vs > 0) & (vs < 0.1)
    print("G16: pixels with 0 < dot(vv, s) < 0.1: %d (per triangle %s), with dot <= 0: %d" % (bend.sum(), [int((bend & (fid == k)).sum()) for k in range(4)],
                                                                                           (vs <= 0).sum()))
    assert bend[:, :30].sum() >= 8 and (vs <= 0).any()
    log = {}

    def texture(tex, uv, filter_mode="linear", boundary_mode="wrap", **kw):
        assert filter_mode == "linear"
        a, c = tex[0].numpy(), uv.numpy()
        if boundary_mode == "cube":
            r = PC.cube_lookup(a, c)
        else:
            assert boundary_mode == "clamp"
            r = PC.lut_lookup(a, c)
        log[len(log)] = boundary_mode
        return torch.from_numpy(r.astype(F32))
    dr.texture = texture
    model = P.PBRModel.__new__(P.PBRModel)
    torch.nn.Module.__init__(model)
    model.light_diffuse, model.light_specular, model.FG_LUT = t(light_d), t(light_s), t(lut)[None]
    diffuse, specular = model.forward(t(eye).reshape(1, 1, 1, 3), t(pos_i)[None], sn[None], t(kd_i)[None], t(ks_i)[None])
    assert sorted(log.values()) == ["clamp", "cube", "cube"]
    rast = full.copy()
    rast[:, 30:] = 0.0
    fix = dict(light_diffuse=light_d, light_specular=light_s, fg_lut=lut, verts=verts, v_nrm=nrm, v_tng=tng, f_nrm=fn, uvs=uvs, faces=faces, rast=rast,
               tex_Kd=kd, tex_Ks=ks, tex_nm=nm, view_position=eye, world_position=pos_i, perturbed_nrm=pert, smooth_nrm=nrm_i, smooth_tng=tng_i, geom_nrm=geom,
               map_Kd=kd_i, map_Ks=ks_i, shading_normal=sn.numpy(), diffuse=diffuse[0].numpy(), specular=specular[0].numpy())
    assert fix["diffuse"].shape == (S, S, 3) and np.isfinite(fix["diffuse"]).all() and np.isfinite(fix["specular"]).all()
    path = os.path.join(out, "g16_normal_map.npz")
    np.savez_compressed(path, **fix)
    print("G16: %d arrays, %d bytes" % (len(fix), os.path.getsize(path)))


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g16(out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
