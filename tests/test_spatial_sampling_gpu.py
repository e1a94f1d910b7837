"""GPU tests of sample_spatial, sample_near_surface, the material lookup at surface samples and texture_sampling (csrc/sampling.hip: utx_sample_offsets,
utx_sample_attrs; csrc/bvh.hip: utx_bvh_closest_point) through the C ABI, against the restatements of oracle/sampling_ref.py and fixture G22 (both pinned on the
CPU in tests/test_spatial_sampling_cpu.py).  Everything float is compared BIT FOR BIT unless a test says why not."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import closest_point_ref as CP, sampling_ref as R

pytestmark = pytest.mark.gpu
g22, tex_bound = R.g22, R.tex_bound
F32 = np.float32
N = 257


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _ico():
    v, f = CP.mesh("ico")
    return v, f, _cu(v), _cu(f, torch.int64)


def _projection_is_closest_point(samples, face_index, face_uvw, vt, ft):
    from unitex_amd.texturetools import ops
    bvh = ops.BVH(vt, ft.to(torch.int32).contiguous())
    o = ops.closest_point(bvh, samples, want=("face", "uvw"))
    assert face_index.dtype == torch.int64 and torch.equal(face_index, o["face"].long()) and torch.equal(face_uvw, o["uvw"])
    # and the tree walk's answer is the restatement's
    ref = CP.closest_point_f32(samples.cpu().numpy(), vt.cpu().numpy(), ft.cpu().numpy())
    assert (face_index.cpu().numpy() == ref[2]).all() and (_bits(face_uvw.cpu().numpy()) == _bits(ref[3])).all()


def test_sample_spatial_is_the_unit_cube_stream_projected_onto_the_mesh():
    from unitex_amd.texturetools import sampling
    v, f, vt, ft = _ico()
    samples, face_index, face_uvw = sampling.sample_spatial(vt, ft, N=N, seed=666)
    assert samples.shape == (N, 3) and (_bits(samples.cpu().numpy()) == _bits(R.uniforms(N, 666, 1))).all()
    assert samples.min() >= 0 and samples.max() < 1          # [0, 1)^3, the reference's torch.rand, not the mesh's box [-1, 1]^3
    _projection_is_closest_point(samples, face_index, face_uvw, vt, ft)
    again = sampling.sample_spatial(vt, ft, N=N, seed=666)
    other = sampling.sample_spatial(vt, ft, N=N, seed=667)
    assert all(torch.equal(a, b) for a, b in zip(again, (samples, face_index, face_uvw))) and not torch.equal(other[0], samples)


def test_sample_near_surface_follows_the_reference_line_by_line():
    from unitex_amd.texturetools import ops, sampling
    v, f, vt, ft = _ico()
    depth, dt = 4, 1.0
    thr = dt * (2.0 / 2 ** depth)
    samples, face_index, face_uvw = sampling.sample_near_surface(vt, ft, N=N, seed=666, distance_threhold=dt, depth=depth)
    # the surface samples are sample_surface's, unchanged: the existing op called directly, on the cum the host code forms
    areas = torch.linalg.cross(vt[ft[:, 1]] - vt[ft[:, 0]], vt[ft[:, 2]] - vt[ft[:, 0]], dim=-1)
    cum = torch.cumsum(torch.norm(areas, p=2, dim=-1).double(), dim=0).float()
    base, bface, buvw = ops.sample_surface(vt, ft.to(torch.int32).contiguous(), cum.contiguous(), int(N * 1.1), 666)
    b2 = sampling.sample_surface(vt, ft, N=int(N * 1.1), seed=666)
    assert torch.equal(b2[0], base) and torch.equal(b2[1], bface.long()) and torch.equal(b2[2], buvw)
    ref_base = R.sample_surface_ref(v, f, cum.cpu().numpy(), int(N * 1.1), 666)
    assert (_bits(base.cpu().numpy()) == _bits(ref_base[0])).all() and (bface.cpu().numpy() == ref_base[1]).all()
    # vertex normals: torch ops (a scatter_add of unit face normals, whose order of summation is torch's) -- a few u of the CPU's
    vn = sampling.unit_normal_vertex_normals(vt, ft)
    assert np.abs(vn.cpu().numpy().astype(np.float64) - R.vertex_normals_unit(v, f)).max() <= 8 * R.U
    want, nrm = R.near_surface_offsets(base.cpu().numpy()[:N], f, bface.cpu().numpy()[:N], buvw.cpu().numpy()[:N], vn.cpu().numpy(), R.uniforms(N, 666, 2), thr)
    assert (_bits(samples.cpu().numpy()) == _bits(want)).all()
    step = np.abs(samples.cpu().numpy().astype(np.float64) - base.cpu().numpy()[:N])
    assert step.max() > 0 and (step <= thr * np.abs(nrm).astype(np.float64) * (1 + 4 * R.U) + 4 * R.U).all()
    assert np.linalg.norm(step, axis=1).max() <= thr * np.linalg.norm(nrm.astype(np.float64), axis=1).max() * (1 + 1e-6)
    _projection_is_closest_point(samples, face_index, face_uvw, vt, ft)
    again = sampling.sample_near_surface(vt, ft, N=N, seed=666, distance_threhold=dt, depth=depth)
    other = sampling.sample_near_surface(vt, ft, N=N, seed=5, distance_threhold=dt, depth=depth)
    assert all(torch.equal(a, b) for a, b in zip(again, (samples, face_index, face_uvw))) and not torch.equal(other[0], samples)
    # a tree handed in gives the same answer as one built inside
    bvh = ops.BVH(vt, ft.to(torch.int32).contiguous())
    assert torch.equal(sampling.sample_near_surface(vt, ft, bvh=bvh, N=N, seed=666, distance_threhold=dt, depth=depth)[0], samples)


def test_sample_offsets_equals_the_reference_run_bit_for_bit():
    """fixture G22(b): the reference's own sample_near_surface, fed the fixture's uniforms; the kernel is fed the same ones through its `uniforms` argument"""
    from unitex_amd.texturetools import ops
    f = g22()
    n, seed, depth, n_surf = (int(x) for x in f["b_params"])
    kw = dict(base=_cu(f["b_base"][:n]), faces=_cu(f["b_faces"]), face_index=_cu(f["b_base_face"][:n]), uvw=_cu(f["b_base_uvw"][:n]),
              vnormal=_cu(f["b_vertex_normals"]), threshold=float(f["b_threshold"][0]))
    got = ops.sample_offsets(n, seed, 2, uniforms=_cu(f["b_uniforms"]), **kw)
    assert (_bits(got.cpu().numpy()) == _bits(f["b_samples"])).all()
    # and with the kernel's own Philox words -- the same numbers
    assert torch.equal(ops.sample_offsets(n, seed, 2, **kw), got)
    # the float64 brute force behind the fixture's cubvh seam (another formula) names the faces the tree walk names, wherever one face alone is nearest
    bvh = ops.BVH(_cu(f["b_verts"]), _cu(f["b_faces"]))
    alone = f["b_face_alone"]
    assert alone.mean() > 0.5 and (ops.closest_point(bvh, got, want=("face",))["face"].cpu().numpy()[alone] == f["b_face"][alone]).all()


def test_sample_attrs_equals_pbr_mesh_call():
    """fixture G22(a): constants and per-vertex attributes bit for bit; the texture within G18's bilinear bound with the reflection fold added (tex_bound)"""
    from unitex_amd.texturetools import sampling
    f = g22()
    for tag, tex in (("8", f["a_tex8"]), ("57", f["a_tex57"])):
        mesh = dict(vertices=_cu(f["a_verts"]), faces=_cu(f["a_faces"]), uvs_2d=_cu(f["a_uvs_2d"]), faces_2d=_cu(f["a_faces"]),
                    albedo=_cu(tex.astype(F32) / F32(255)), metallic=_cu(f["a_metallic"]), roughness=_cu(f["a_roughness"]))
        got = sampling.pbr_attributes(mesh, _cu(f["a_face_idx"]), _cu(f["a_uvw"]))
        assert {k: tuple(t.shape) for k, t in got.items()} == {"albedo": (64, 3), "metallic": (64, 1), "roughness": (64, 1), "bump": (64, 3)}
        assert (_bits(got["roughness"].cpu().numpy()) == _bits(f["a_out%s_roughness" % tag])).all()
        assert (_bits(got["metallic"].cpu().numpy()) == _bits(f["a_out%s_metallic" % tag])).all()
        assert (_bits(got["bump"].cpu().numpy()) == _bits(f["a_out%s_bump" % tag])).all()
        err = np.abs(got["albedo"].cpu().numpy().astype(np.float64) - f["a_out%s_albedo" % tag]).max()
        print("texture %s: %.2f u (bound %.0f u)" % (tag, err / R.U, tex_bound(tex) / R.U))
        assert err <= tex_bound(tex)
    # no material at all: PBRDefault's values
    bare = sampling.pbr_attributes(dict(vertices=mesh["vertices"], faces=mesh["faces"]), _cu(f["a_face_idx"]), _cu(f["a_uvw"]))
    assert (bare["albedo"] == 0).all() and (bare["metallic"] == 0).all() and (bare["roughness"] == 1).all() and (bare["bump"] == 0).all()
    with pytest.raises(NotImplementedError):
        sampling.sample_pbr_mesh([mesh, mesh], N=4)


@pytest.mark.parametrize("H,W", R.REFLECT_SIZES)
def test_texture_lookup_is_the_float32_restatement_bit_for_bit(H, W):
    """utx_sample_attrs' texture lookup against oracle.sampling_ref.texture_attr in float32 (pinned against torch's grid_sample in tests/test_spatial_sampling_cpu.py),
    by uint32 view: C = 1, 3 and 4 channels in one launch, N = 257 (one block and one thread), the uv of reflect_case, +-1e12 (a flip count past int32) included"""
    from unitex_amd.texturetools import ops
    tex, f2, uvs, fi, uvw = R.reflect_case(H, W, N)
    got = ops.sample_attrs({"c%d" % c: _cu(t) for c, t in tex.items()}, _cu(fi), _cu(uvw), faces_2d=_cu(f2), uvs_2d=_cu(uvs))
    for c, t in tex.items():
        want = R.texture_attr(t, uvs, f2, fi, uvw, F32)[0]
        differ = np.flatnonzero((_bits(got["c%d" % c].cpu().numpy()) != _bits(want)).any(1))
        assert want.shape == (N, c) and len(differ) == 0, (c, uvs[differ[:8]].tolist())


def test_texture_sampling_round_trip(tmp_path):
    from unitex_amd.texturetools import meshes, sampling
    verts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    uvs = np.array([[0.1, 0.1], [0.9, 0.1], [0.9, 0.9], [0.1, 0.9]], F32)
    tex = np.random.default_rng(3).integers(0, 256, (6, 9, 3), dtype=np.uint8)
    glb, ply = str(tmp_path / "quad.glb"), str(tmp_path / "out" / "cloud.ply")
    meshes.save_glb(glb, verts, faces, uvs, tex)
    log = sampling.texture_sampling(glb, ply, N=N)
    assert set(log) == {"load scene", "move mesh to gpu", "sample on mesh", "move samples to cpu", "export point cloud"}
    pts, pf, _, col = meshes.load_ply(ply, faces_required=False, vertex_colors=True)
    lv, lf, luv, ltex = meshes.load_glb(glb)
    from types import SimpleNamespace
    mesh = sampling.pbr_mesh_from_textured(SimpleNamespace(vertices=lv, faces=lf, uv=luv, texture=ltex))
    samples, face_index, attr = sampling.sample_pbr_mesh(mesh, N=N, seed=666)
    assert pts.shape == (N, 3) and len(pf) == 0 and (_bits(pts) == _bits(samples.cpu().numpy())).all()
    a = attr["albedo"].cpu().numpy()
    want = np.round(np.clip(a, F32(0), F32(1)) * F32(255)).astype(np.uint8)          # round(clamp(albedo, 0, 1) * 255) in float32, halves to even
    assert col.dtype == np.uint8 and (col == want).all()
    # the colours are the texture's: every sample lies inside the quad's chart, so its colour lies within the texels' range, and the cloud is not one colour
    assert col.min() >= tex.min() and col.max() <= tex.max() and len(np.unique(col, axis=0)) > 16
    assert (attr["metallic"] == 0).all() and (attr["roughness"] == 1).all()
    # a .glb without a material is an untextured mesh: PBRDefault's albedo, a black cloud at the same points
    import json
    import struct
    js, binc = meshes._glb_chunks(glb)
    for k in ("materials", "textures", "images", "samplers"):
        js.pop(k)
    js["meshes"][0]["primitives"][0].pop("material")
    head = json.dumps(js, separators=(",", ":")).encode()
    head += b" " * ((-len(head)) % 4)
    bare, ply2 = str(tmp_path / "bare.glb"), str(tmp_path / "bare.ply")
    with open(bare, "wb") as fh:
        fh.write(struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(head) + 8 + len(binc)) + struct.pack("<II", len(head), 0x4E4F534A) + head +
                 struct.pack("<II", len(binc), 0x004E4942) + binc)
    sampling.texture_sampling(bare, ply2, N=N)
    pts2, _, _, col2 = meshes.load_ply(ply2, faces_required=False, vertex_colors=True)
    assert (_bits(pts2) == _bits(pts)).all() and (col2 == 0).all()


def test_error_codes():
    from unitex_amd.texturetools.ops import get_ctx
    ctx = get_ctx(0)
    lib = ctx.lib
    out = torch.zeros(8, 3, device="cuda")
    o, z = C.c_void_p(out.data_ptr()), C.c_void_p(0)
    off = lambda base, n, sid, outp: lib.utx_sample_offsets(ctx.handle, base, z, 0, z, z, z, z, n, 1, sid, C.c_float(0.5), outp, ctx.stream())
    assert off(z, 0, 1, z) == 0 and off(z, 8, 1, o) == 0
    assert off(z, 8, 0, o) == -2 and off(z, -1, 1, o) == -2 and off(z, 2 ** 31, 1, o) == -2 and off(z, 8, 1, z) == -2
    assert off(o, 8, 2, o) == -2          # a base without faces, indices, weights and normals
    fi, w = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, 3, device="cuda")
    const = torch.ones(3, device="cuda")
    src, dst = (C.c_void_p * 1)(const.data_ptr()), (C.c_void_p * 1)(out.data_ptr())
    att = lambda n_attr, dims, n=8: lib.utx_sample_attrs(ctx.handle, z, z, z, 1, C.c_void_p(fi.data_ptr()), C.c_void_p(w.data_ptr()), n, n_attr, src,
                                                         (C.c_int * 4)(*dims), dst, ctx.stream())
    assert att(1, (0, 3, 0, 0)) == 0
    torch.cuda.synchronize()
    assert (out == 1).all()
    assert att(0, (0, 3, 0, 0)) == -2 and att(5, (0, 3, 0, 0)) == -2 and att(1, (3, 3, 0, 0)) == -2 and att(1, (0, 0, 0, 0)) == -2 and att(1, (0, 17, 0, 0)) == -2
    assert att(1, (1, 3, 0, 0)) == -2 and att(1, (2, 3, 4, 4)) == -2          # a vertex attribute without faces, a texture without uvs
    assert att(1, (0, 3, 0, 0), n=-1) == -2
