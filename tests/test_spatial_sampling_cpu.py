"""CPU pins of the sampling restatements of tests/closest_point_ref.py against fixture G22 (tests/golden/make_golden_spatial_sampling.py: the reference's own
PBRMesh.__call__ and sample_near_surface on CPU tensors), before tests/test_spatial_sampling_gpu.py leans on them."""
import numpy as np

from tests import closest_point_ref as R

F32 = np.float32


g22, tex_bound = R.g22, R.tex_bound


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_near_surface_arithmetic_equals_the_reference_bit_for_bit():
    f = g22()
    N, seed, depth, n_surf = (int(x) for x in f["b_params"])
    assert n_surf == int(N * 1.1) and f["b_base"].shape == (n_surf, 3)
    assert (_bits(f["b_uniforms"]) == _bits(R.uniforms(N, seed, 2))).all()
    thr = float(f["b_threshold"][0])
    assert thr == 1.0 * (2.0 / 2 ** depth)
    got, nrm = R.near_surface_offsets(f["b_base"][:N], f["b_faces"], f["b_base_face"][:N], f["b_base_uvw"][:N], f["b_vertex_normals"], f["b_uniforms"], thr)
    assert (_bits(got) == _bits(f["b_samples"])).all()
    # within threshold * max|normal| per component of the surface sample, and not on it
    step = np.abs(f["b_samples"].astype(np.float64) - f["b_base"][:N])
    assert step.max() > 0 and (step <= thr * np.abs(nrm).astype(np.float64) * (1 + 4 * R.U) + 4 * R.U).all()
    # the vertex normals: the normalised sum of the UNIT face normals -- on the icosphere NOT the area-weighted ones, and of unit length
    vn = R.vertex_normals_unit(f["b_verts"], f["b_faces"])
    assert np.abs(vn.astype(np.float64) - f["b_vertex_normals"]).max() <= 4 * R.U
    assert np.abs(np.linalg.norm(vn.astype(np.float64), axis=1) - 1).max() <= 4 * R.U
    # the faces the float64 brute force named behind the cubvh seam (another formula) are the float32 restatement's
    dist, d2, face, uvw, q = R.closest_point_f32(f["b_samples"], f["b_verts"], f["b_faces"])
    alone = f["b_face_alone"]
    assert alone.mean() > 0.5 and (face[alone] == f["b_face"][alone]).all()
    # where several faces are nearest (outside a convex edge) either may be named: the distances agree
    assert np.abs(dist.astype(np.float64) - R.face_dist_f64(f["b_samples"], f["b_verts"], f["b_faces"], f["b_face"])).max() <= R.BOUND_U * R.U * R.scene_scale(f["b_samples"], f["b_verts"])


def test_material_lookup_equals_the_reference():
    f = g22()
    fi, uvw = f["a_face_idx"], f["a_uvw"]
    worst = {}
    for tag, tex in (("8", f["a_tex8"]), ("57", f["a_tex57"])):
        assert (f["a_out%s_metallic" % tag] == f["a_metallic"][None]).all() and (f["a_out%s_bump" % tag] == 0).all()
        assert (_bits(R.vertex_attr(f["a_roughness"], f["a_faces"], fi, uvw)) == _bits(f["a_out%s_roughness" % tag])).all()
        got, uv, ix, iy = R.texture_attr(tex.astype(np.float64) / 255.0, f["a_uvs_2d"], f["a_faces"], fi, uvw)
        assert (np.abs(uv) > 1).any() and (uv < -1).any()          # the uv is the grid coordinate as it stands: reflection happens
        err = np.abs(got - f["a_out%s_albedo" % tag].astype(np.float64)).max()
        worst[tag] = err / R.U
        assert err <= tex_bound(tex), (tag, err / R.U)
    print("texture lookup, restatement in float64 against torch's grid_sample: %s u (bounds %.0f u and %.0f u)" % (
        ", ".join("%s: %.2f" % kv for kv in worst.items()), tex_bound(f["a_tex8"]) / R.U, tex_bound(f["a_tex57"]) / R.U))
    # the quirk is real: with the uv mapped from [0, 1] to [-1, 1] first the values are others
    mapped = R.texture_attr(f["a_tex8"].astype(np.float64) / 255.0, f["a_uvs_2d"] * F32(2) - F32(1), f["a_faces"], fi, uvw)[0]
    assert np.abs(mapped - f["a_out8_albedo"]).max() > 0.05


def test_sample_attrs_refuses_a_uv_table_without_its_index_before_any_device_call():
    """faces_2d and uvs_2d go together (the kernel reads one through the other): one without the other is -2 from the C ABI, refused before anything touches a
    device -- so it runs here, with made-up addresses that are never read -- and a ValueError from ops"""
    import ctypes as C

    import pytest
    from unitex_amd import _lib
    from unitex_amd.texturetools import ops
    lib = _lib.load_library()
    some, z = C.c_void_p(4096), C.c_void_p(0)
    src, dst = (C.c_void_p * 1)(4096), (C.c_void_p * 1)(4096)
    call = lambda f2, uv, dims: lib.utx_sample_attrs(None, some, f2, uv, 4, some, some, 8, 1, src, (C.c_int * 4)(*dims), dst, None)
    for dims in ((0, 3, 0, 0), (1, 3, 0, 0), (2, 3, 4, 4)):
        assert call(some, z, dims) == -2 and call(z, some, dims) == -2
    assert call(z, z, (2, 3, 4, 4)) == -2          # a texture without both
    with pytest.raises(ValueError, match="go together"):
        ops.sample_attrs({"a": None}, None, None, faces_2d=object(), uvs_2d=None)
    with pytest.raises(ValueError, match="go together"):
        ops.sample_attrs({"a": None}, None, None, faces_2d=None, uvs_2d=object())
