"""Tangent-space normal maps, CPU side: the fp64 restatement of bsdf_prepare_shading_normal (oracle/pbr_ref.py: shading_normal, chained to pbr_forward,
and the error bounds the GPU tests hold the kernels to, with their derivation) proven against the reference's own torch code (fixture G16,
tests/golden/make_golden_normal_map.py) and cross-checked against the reference's own fp32 distance from the restatement; meshes.vertex_tangents; the
argument check of ops.pbr_shade."""

import numpy as np
import pytest

from oracle.pbr_ref import F32, g16_oracle, load_g16, shading_normal
from oracle.pixel_ref import unit


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
    assert away.sum() > len(verts) // 2 and ((t * unit(lon)).sum(-1)[away] > 0).all()


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
