"""Tangent-space normal maps, CPU side: the fp64 restatement of bsdf_prepare_shading_normal (two-sided, OpenGL convention; the rule in
include/unitex_hip.h), proven against the reference's own torch code (fixture G16, tests/golden/make_golden_normal_map.py) and chained to
tests/test_pbr_cpu.pbr_forward; the error bounds the GPU tests hold the kernels to (derived here by counting roundings, cross-checked against the
reference's own fp32 distance from the restatement); meshes.vertex_tangents; the argument check of ops.pbr_shade.

Bounds, in units of u = 2^-24 (half an ulp of a value in [1, 2), as in test_pbr_gpu.test_g15_forward_and_fused_shade), absolute, first order, every
rounding taken in the same direction.  c = |cross(st, sn)|, r = |st p.x - b p.y + sn max(p.z, 0)|, both of the fp64 restatement:
  a normalised vector (dot 3, sqrt 1, divide 1)                                   5 u         (vv: one more for eye - pos, 6 u)
  cross(st, sn), per component two products of factors good to 5 u and a sum      23 u, as a vector 40 u
  b = cross / |cross|                                                              40 u / c + 5 u
  s_raw (|p| <= 1: 5 u on st and sn, |p.y| times b's, 3 products, 2 sums)          40 u (1 + |p.y| / c)
  s = s_raw / |s_raw|                                                              ds = 40 u (1 + |p.y| / c) / r + 5 u
  t = clamp(dot(vv, s) / 0.1)   (ds + 6 u + 3 u for the dot, times 10, the divide)  dt = 10 (ds + 10 u) + 2 u, and 0 where the fp64 dot / 0.1 lies
                                                                                   farther than dt outside [0, 1]: both sides clamp to the same 0 or 1
  out = g + t (s - g)                                                              (1 + |g|) dt + ds + 6 u max(1, |g|)
  r = 0 exactly (p.x = p.y = max(p.z, 0) = 0, or the frame itself is zero): the three products are exact zeros on both sides, s = 0, t = 0, out = g: ds = dt = 0
An ill-conditioned pixel (tangent nearly parallel to the normal, a perturbation near zero) gets the wider bound its own c and r give it, no pixel is
left out.  Through the shading (lights of N^2 faces with texel contrast C and maximum M, an R^2 table with contrast <= 1, kd <= 1, roughness exact):
  dn = d(out) / |out| + 5 u on the unit normal;  a direction error d moves a face coordinate by <= 2 sqrt(3) d, N / 2 texels per unit, two axes, C per
  texel: K d with K = 2 * 2 sqrt(3) * (N / 2) * C;  a lookup that snaps on one side only (rule 2 of the cube lookup) jumps by <= N 2^-21 C per axis
  diffuse  = kd * light_diffuse[n]:                       K dn + 2 N 2^-21 C
  specular = (ks FG.x + FG.y) * light_specular[wi]:       wi = 2 (wo.n) n - wo moves by 4 dn, the coefficient is <= 1.5: 1.5 (4 K dn + 2 N 2^-21 C);
             FG[c = wo.n] moves by R dn per entry, the coefficient by 1.5 R dn, times M
plus, against another evaluation of the whole chain, the 16 ulp of each output's maximum that G15 grants PBRModel.forward itself."""
import os

import numpy as np
import pytest

from tests import test_pbr_cpu as PC

GOLD = PC.GOLD
F32 = np.float32
U = PC.U
_cache = {}


def load_g16():
    if "f" not in _cache:
        _cache["f"] = dict(np.load(os.path.join(GOLD, "g16_normal_map.npz"), allow_pickle=False))
    return _cache["f"]


def _n(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-12)


def shading_normal(view_pos, pos, p, smooth_nrm, smooth_tng, geom_nrm, parts=False):
    """bsdf_prepare_shading_normal(two_sided_shading=True, opengl=True) in fp64 -> out [...,3] (, the intermediates the bounds need)"""
    f = lambda a: np.asarray(a, np.float64)
    view_pos, pos, p, g = f(view_pos), f(pos), f(p), f(geom_nrm)
    sn, st, vv = _n(f(smooth_nrm)), _n(f(smooth_tng)), _n(view_pos - pos)
    c = np.cross(st, sn)
    b = _n(c)
    s_raw = st * p[..., 0:1] - b * p[..., 1:2] + sn * np.maximum(p[..., 2:3], 0.0)
    s = _n(s_raw)
    front = (g * vv).sum(-1, keepdims=True) > 0
    s, g = np.where(front, s, -s), np.where(front, g, -g)
    t_raw = (vv * s).sum(-1, keepdims=True) / 0.1
    out = g + np.clip(t_raw, 0.0, 1.0) * (s - g)
    if parts:
        return out, dict(c=np.linalg.norm(c, axis=-1), r=np.linalg.norm(s_raw, axis=-1), t_raw=t_raw[..., 0], gl=np.linalg.norm(g, axis=-1), py=np.abs(p[..., 1]),
                         gdot=(f(geom_nrm) * vv).sum(-1))
    return out


def shading_normal_bound(parts):
    """per-pixel absolute bound on a fp32 evaluation of the rule against the fp64 one (module docstring)"""
    tiny = 1e-300
    ds = 40 * U * (1 + parts["py"] / np.maximum(parts["c"], tiny)) / np.maximum(parts["r"], tiny) + 5 * U
    ds = np.where(parts["r"] == 0, 0.0, ds)
    dt = 10 * (ds + 10 * U) + 2 * U
    dt = np.where((parts["t_raw"] <= -dt) | (parts["t_raw"] >= 1 + dt) | (parts["r"] == 0), 0.0, dt)
    return (1 + parts["gl"]) * dt + ds + 6 * U * np.maximum(1.0, parts["gl"])


def shade_bounds(d_out, out, N, contrast, light_max, R):
    """(diffuse, specular) per-pixel bounds from the bound d_out on the un-normalised shading normal `out` (module docstring), without the 16 ulp"""
    dn = d_out / np.maximum(np.linalg.norm(out, axis=-1), 1e-300) + 5 * U
    K = 2 * 2 * np.sqrt(3.0) * (N / 2) * contrast
    snap = 2 * N * 2.0 ** -21 * contrast
    return K * dn + snap, 1.5 * (4 * K * dn + snap) + 1.5 * R * dn * light_max


def g16_oracle():
    """the restatement on G16's dense inputs, once: out, parts, bound, diffuse, specular, their bounds"""
    if "o" not in _cache:
        f = load_g16()
        out, parts = shading_normal(f["view_position"], f["world_position"], f["perturbed_nrm"], f["smooth_nrm"], f["smooth_tng"], f["geom_nrm"], parts=True)
        bound = shading_normal_bound(parts)
        d, s = PC.pbr_forward(f["view_position"], f["world_position"], out, f["map_Kd"], f["map_Ks"], f["light_diffuse"], f["light_specular"], f["fg_lut"])
        bd, bs = shade_bounds(bound, out, 8, 2.0, 4.0, 16)
        ulp = lambda x: float(np.spacing(F32(np.abs(x).max())))
        _cache["o"] = dict(out=out, parts=parts, bound=bound, diffuse=d, specular=s, bound_diffuse=bd + 16 * ulp(d), bound_specular=bs + 16 * ulp(s))
    return _cache["o"]


# ---------------------------------------------------------------------------------------------------------------- tests
def test_g16_has_the_cases():
    f = load_g16()
    o = g16_oracle()
    p, parts = f["perturbed_nrm"], o["parts"]
    cov = f["rast"][..., 3] > 0
    assert cov.any() and not cov.all() and set(np.unique(f["rast"][..., 3])) == {0.0, 1.0, 2.0, 3.0, 4.0}
    assert np.abs(parts["gdot"]).min() >= 1e-3, "fp32 and fp64 decide the flip alike"
    assert (parts["gdot"][cov] < 0).any() and (parts["gdot"][cov] > 0).any(), "a triangle faces away from the eye"
    bend = (parts["t_raw"] > 0) & (parts["t_raw"] < 1) & cov
    assert bend.sum() >= 8, "the bend region 0 < dot(vv, s) < 0.1"
    assert (p[12, 12] == 0).all() and (p[..., 2] < 0).any() and (p == np.array([0, 0, 1], F32)).all(-1).any()
    assert np.abs(np.linalg.norm(f["smooth_nrm"], axis=-1) - 1).max() > 0.1 and np.abs(np.linalg.norm(f["smooth_tng"], axis=-1) - 1).max() > 0.1
    assert np.array_equal(f["v_tng"][3] * F32(2.0), f["v_nrm"][3]), "one vertex's tangent is parallel to its normal"
    assert parts["c"].min() < 0.1, "and the pixels near it are ill-conditioned (|cross(st, sn)| small)"


def test_restatement_reproduces_the_reference():
    """G16's shading normal, diffuse and specular are the reference's own fp32 torch; each lies inside the derived bound of the fp64 restatement at EVERY pixel
    (the cross-check of the derivation: a reference outside it would mean the count is wrong).  Measured: shading normal max 7.3e-7 absolute, at most 0.023 of
    its pixel's bound; diffuse 1.7e-6 absolute (5.7e-7 of the maximum), 0.0011 of its bound; specular 1.5e-5 (3.5e-6 of the maximum), 0.0025 of its bound."""
    f, o = load_g16(), g16_oracle()
    err = np.abs(o["out"] - f["shading_normal"]).max(-1)
    print("shading normal: reference fp32 vs fp64 restatement: max %.3g, max error / bound %.3g (bound %.3g .. %.3g)"
          % (err.max(), (err / o["bound"]).max(), o["bound"].min(), o["bound"].max()))
    assert (err <= o["bound"]).all()
    for name in ("diffuse", "specular"):
        e = np.abs(o[name] - f[name]).max(-1)
        print("%s: reference fp32 vs fp64 restatement: max %.3g (%.3g of the maximum), max error / bound %.3g"
              % (name, e.max(), e.max() / np.abs(f[name]).max(), (e / o["bound_" + name]).max()))
        assert (e <= o["bound_" + name]).all(), name
    assert np.isfinite(o["out"]).all() and np.isfinite(o["diffuse"]).all() and np.isfinite(o["specular"]).all()


def test_restatement_degenerate_inputs_are_finite():
    """zero tangent, tangent parallel to the normal, zero perturbation, negative p.z: finite at every stage, and out = g where s = 0"""
    eye, pos, n, g = np.array([0.0, 0.0, 3.0]), np.zeros(3), np.array([0.0, 0.0, 2.0]), np.array([0.0, 0.0, 1.0])
    for p, t in (((0.3, 0.2, 0.5), (0, 0, 0)), ((0.3, 0.2, 0.5), (0, 0, 1)), ((0, 0, 0), (1, 0, 0)), ((0.3, 0.2, -0.7), (1, 0, 0)), ((0, 0, -1.0), (0, 0, 0))):
        out = shading_normal(eye, pos, np.array(p, np.float64), n, np.array(t, np.float64), g)
        assert np.isfinite(out).all()
    assert np.array_equal(shading_normal(eye, pos, np.zeros(3), n, np.array([1.0, 0, 0]), g), g)


def test_vertex_tangents_plane():
    from unitex_amd.texturetools.meshes import vertex_tangents
    k = 5
    gx, gy = np.meshgrid(np.arange(k) / (k - 1.0), np.arange(k) / (k - 1.0), indexing="xy")
    verts = np.stack([gx, gy, np.zeros_like(gx)], -1).reshape(-1, 3).astype(F32)
    idx = lambda j, i: j * k + i
    faces = np.asarray([[idx(j, i), idx(j, i + 1), idx(j + 1, i + 1)] for j in range(k - 1) for i in range(k - 1)] +
                       [[idx(j, i), idx(j + 1, i + 1), idx(j + 1, i)] for j in range(k - 1) for i in range(k - 1)], np.int32)
    t = vertex_tangents(verts, faces, verts[:, :2], np.tile(np.array([0, 0, 1], F32), (k * k, 1)))
    assert t.dtype.is_floating_point and tuple(t.shape) == (k * k, 3) and str(t.dtype) == "torch.float32"
    assert np.array_equal(t.numpy(), np.tile(np.array([1, 0, 0], F32), (k * k, 1)))


def test_vertex_tangents_uv_sphere():
    import torch
    from unitex_amd.texturetools import meshes
    from unitex_amd.texturetools.video import _vertex_normals
    verts, faces, uvs = meshes.make_bumpy_sphere(32, 16)
    n = _vertex_normals(torch.from_numpy(verts), torch.from_numpy(faces), "angle")
    t = meshes.vertex_tangents(verts, faces, uvs, n).numpy().astype(np.float64)
    n = n.numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(t, axis=-1) - 1).max() <= 1e-6
    assert np.abs((t * n).sum(-1)).max() <= 1e-6
    lon = np.stack([-verts[:, 2], np.zeros(len(verts)), verts[:, 0]], -1).astype(np.float64)
    away = np.abs(verts[:, 1]) < 0.8 * np.abs(verts[:, 1]).max()
    assert away.sum() > len(verts) // 2 and ((t * _n(lon)).sum(-1)[away] > 0).all()


def test_vertex_tangents_degenerate():
    from unitex_amd.texturetools.meshes import vertex_tangents
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [5, 5, 5], [2, 0, 0]], F32)          # vertex 4 is unreferenced
    faces = np.array([[0, 1, 2], [1, 3, 5]], np.int32)                                                  # face 1 has no UV area
    uvs = np.array([[0, 0], [1, 0], [0, 1], [1, 0], [0.5, 0.5], [1, 0]], F32)
    nrm = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 2], [0, 0, 0], [1, 1, 1]], F32)            # and a zero normal
    t = vertex_tangents(verts, faces, uvs, nrm).numpy().astype(np.float64)
    assert np.isfinite(t).all() and np.abs(np.linalg.norm(t, axis=-1) - 1).max() <= 1e-6
    assert np.abs((t * nrm).sum(-1)).max() <= 1e-6
    assert np.array_equal(t[0], [1, 0, 0]) and np.array_equal(t[3], [0, 1, 0]), "face 0's tangent; the fallback cross(n, x axis) for (0, 0, 1)"


def test_pbr_shade_refuses_a_partial_normal_map(monkeypatch):
    """the argument check comes before the library is touched: get_ctx is replaced by a stub that fails the test if it is reached"""
    from unitex_amd.texturetools import ops

    def no_ctx(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "get_ctx", no_ctx)
    x = object()
    for kw in (dict(v_tng=x), dict(f_nrm=x), dict(normal_map=x), dict(v_tng=x, f_nrm=x), dict(v_tng=x, normal_map=x), dict(f_nrm=x, normal_map=x)):
        with pytest.raises(ValueError):
            ops.pbr_shade(*([None] * 11), **kw)
