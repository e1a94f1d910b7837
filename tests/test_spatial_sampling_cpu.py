"""CPU pins of the sampling restatements of oracle/sampling_ref.py against fixture G22 (tests/golden/make_golden_spatial_sampling.py: the reference's own
PBRMesh.__call__ and sample_near_surface on CPU tensors), before tests/test_spatial_sampling_gpu.py leans on them."""
import numpy as np
import pytest
import torch

from oracle import closest_point_ref as CP, sampling_ref as R
from oracle.pixel_ref import grid_unnormalize

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
    dist, d2, face, uvw, q = CP.closest_point_f32(f["b_samples"], f["b_verts"], f["b_faces"])
    alone = f["b_face_alone"]
    assert alone.mean() > 0.5 and (face[alone] == f["b_face"][alone]).all()
    # where several faces are nearest (outside a convex edge) either may be named: the distances agree
    assert np.abs(dist.astype(np.float64) - CP.face_dist_f64(f["b_samples"], f["b_verts"], f["b_faces"], f["b_face"])).max() <= CP.BOUND_U * R.U * CP.scene_scale(f["b_samples"], f["b_verts"])


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


@pytest.mark.parametrize("H,W", R.REFLECT_SIZES)
def test_float32_texture_lookup_against_grid_sample(H, W):
    """the float32 restatement that tests/test_spatial_sampling_gpu.py holds utx_sample_attrs' texture lookup to bit for bit, on that test's inputs, against torch's
    CPU grid_sample(reflection): within 4 u max|texel|, the bound of tests/test_vertex_bake_cpu.py's reflection lookup.  +-1e12 is left to the GPU test"""
    tex, f2, uvs, fi, uvw = R.reflect_case(H, W)
    assert len(fi) == 257 and (np.abs(uvs) == F32(R.REFLECT_HUGE)).any(1).sum() == 4
    keep = (np.abs(uvs) < R.REFLECT_HUGE).all(1)
    grid = torch.from_numpy(uvs[keep])[None, :, None]
    for c, t in tex.items():
        got, uv, ix, iy = R.texture_attr(t, uvs, f2, fi, uvw, F32)
        assert t.shape == (H, W, c) and t.min() < 0 and np.isfinite(got).all()        # negative texels; 1e12 lands on the texture too
        assert (_bits(uv) == _bits(uvs)).all()                                        # weights (1, 0, 0): the hand-made uv reaches the lookup as it stands
        flips = np.floor(np.abs(grid_unnormalize(uvs[keep, 0], W) + F32(0.5)) / F32(W))
        assert (ix[keep] == W - 1).any() and (iy[keep] == H - 1).any() and {0, 1, 2, 3, 4} <= set(flips.astype(int).tolist())      # the absent tap; odd and even flips
        want = torch.nn.functional.grid_sample(torch.from_numpy(t).permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="reflection", align_corners=False)
        err = np.abs(got[keep].astype(np.float64) - want[0, :, :, 0].T.numpy()).max()
        print("%d x %d x %d: %.2f u (bound %.2f u)" % (H, W, c, err / R.U, 4 * np.abs(t).max()))
        assert err <= 4 * R.U * np.abs(t).max()


def test_sample_attrs_refuses_a_uv_table_without_its_index_before_any_device_call():
    """faces_2d and uvs_2d go together (the kernel reads one through the other): one without the other is -2 from the C ABI, refused before anything touches a
    device -- so it runs here, with made-up addresses that are never read -- and a ValueError from ops"""
    import ctypes as C

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
