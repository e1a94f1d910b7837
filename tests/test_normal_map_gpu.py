"""Tangent-space normal maps on the GPU (csrc/pbr.hip: utx_pbr_shading_normal, utx_pbr_shade_nm) against the reference's own code (fixture G16) and the fp64
restatement of oracle/pbr_ref.py, with the per-pixel bounds derived in that module's docstring (the same bounds its CPU test holds the
reference's own fp32 result to)."""
import numpy as np
import pytest
import torch

from oracle import pbr_ref as PC
from oracle import video_types_ref as VC

pytestmark = pytest.mark.gpu
F32 = np.float32
U = PC.U


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _ulp(x):
    return float(np.spacing(F32(np.abs(x).max())))


def test_g16_shading_normal():
    """utx_pbr_shading_normal on the dense inputs the reference saw: within the derived per-pixel bound of the reference's own output (the bound is the one for
    a fp32 evaluation against the fp64 restatement; the kernel is held to it against the reference directly, which is stricter), every pixel."""
    from unitex_amd.texturetools import ops
    f, o = PC.load_g16(), PC.g16_oracle()
    d = lambda k: _cu(f[k].reshape(-1, 3))
    got = ops.pbr_shading_normal(_cu(f["view_position"]), d("world_position"), d("perturbed_nrm"), d("smooth_nrm"), d("smooth_tng"), d("geom_nrm"))
    got = got.cpu().numpy().reshape(32, 32, 3)
    assert np.isfinite(got).all()
    e_ref, e_64 = np.abs(got - f["shading_normal"]).max(-1), np.abs(got - o["out"]).max(-1)
    print("G16 shading normal: vs the reference max %.3g (%.3g of the bound), vs fp64 max %.3g (%.3g of the bound)"
          % (e_ref.max(), (e_ref / o["bound"]).max(), e_64.max(), (e_64 / o["bound"]).max()))
    assert (e_ref <= o["bound"]).all() and (e_64 <= o["bound"]).all()
    assert np.array_equal(got[12, 12], f["geom_nrm"][12, 12]), "a zero perturbation returns the geometric normal itself"
    eye = np.broadcast_to(f["view_position"], (1024, 3)).copy()
    again = ops.pbr_shading_normal(_cu(eye), d("world_position"), d("perturbed_nrm"), d("smooth_nrm"), d("smooth_tng"), d("geom_nrm"))
    assert np.array_equal(again.cpu().numpy().reshape(32, 32, 3), got), "view_stride 3 and 0 agree bit for bit"


def test_g16_fused_shade():
    """utx_pbr_shade_nm on G16's mesh-level inputs: diffuse alone and specular alone against the fp64 restatement within the per-pixel bounds (the shading
    normal's bound through the lookups, plus G15's 16 ulp of the maximum for PBRModel.forward itself), uint8 within 1, the background exact."""
    from unitex_amd.texturetools import ops
    f, o = PC.load_g16(), PC.g16_oracle()
    bg = (0.25, 0.5, 0.75)
    args = (_cu(f["rast"]), _cu(f["faces"], torch.int32), _cu(f["verts"]), _cu(f["v_nrm"]), _cu(f["uvs"]), _cu(f["tex_Kd"]), _cu(f["tex_Ks"]), f["view_position"].tolist(),
            _cu(f["light_diffuse"]), _cu(f["light_specular"]), _cu(f["fg_lut"]))
    nm = dict(v_tng=_cu(f["v_tng"]), f_nrm=_cu(f["f_nrm"]), normal_map=_cu(f["tex_nm"]), bg=bg, want_rgba=True)
    _, fd = ops.pbr_shade(*args, lambda_diffuse=1.0, lambda_specular=0.0, **nm)
    _, fs = ops.pbr_shade(*args, lambda_diffuse=0.0, lambda_specular=1.0, **nm)
    u8, frgb = ops.pbr_shade(*args, **nm)
    cov = f["rast"][..., 3] > 0
    assert cov.any() and not cov.all()
    for name, fused in (("diffuse", fd), ("specular", fs)):
        got = fused.cpu().numpy()
        assert np.isfinite(got).all()
        e, e_ref = np.abs(got[..., :3] - o[name]).max(-1)[cov], np.abs(got[..., :3] - f[name]).max(-1)[cov]
        print("G16 %s through the fused frame: vs fp64 max %.3g (%.2f ulp of the maximum, %.3g of the bound), vs the reference max %.3g"
              % (name, e.max(), e.max() / _ulp(o[name]), (e / o["bound_" + name][cov]).max(), e_ref.max()))
        assert (e <= o["bound_" + name][cov]).all(), name
        assert (got[~cov][:, :3] == np.array(bg, F32)).all() and np.array_equal(got[..., 3], cov.astype(F32))
    frgb, u8 = frgb.cpu().numpy(), u8.cpu().numpy()
    assert (frgb[~cov][:, :3] == np.array(bg, F32)).all() and (u8[~cov] == (np.array(bg, F32) * F32(255.0)).astype(np.uint8)).all()
    want = (np.clip(f["diffuse"] + f["specular"], 0, 1) * F32(255.0)).astype(np.uint8)
    assert np.abs(u8.astype(np.int32) - want.astype(np.int32))[cov].max() <= 1
    # the map matters on this fixture: without it the frame is another one
    _, plain = ops.pbr_shade(*args, bg=bg, want_rgba=True)
    assert not np.array_equal(plain.cpu().numpy(), frgb)


def _torus():
    """the torus of test_pbr_gpu.test_torus_frame.  Its faces are wound clockwise seen from outside (cross(v1 - v0, v2 - v0) opposes its vertex normals), which
    the two-sided rule reads as 'every visible face is a back face'; reversed here, so that geometric and vertex normals agree as on a mesh made for shading."""
    f = dict(VC.load())
    f["faces"] = np.ascontiguousarray(f["faces"][:, ::-1])
    v = f["verts"].astype(np.float64)
    fn = np.cross(v[f["faces"][:, 1]] - v[f["faces"][:, 0]], v[f["faces"][:, 2]] - v[f["faces"][:, 0]])
    assert ((fn * f["v_nrm"][f["faces"]].mean(1)).sum(-1) > 0).all()
    return f


def _torus_frame(size=64):
    from unitex_amd.texturetools import camera, meshes, ops
    f = _torus()
    rng = np.random.default_rng(9)
    ld, ls, lut = (rng.uniform(0, 2, (6, 8, 8, 3)).astype(F32), rng.uniform(0, 2, (6, 8, 8, 3)).astype(F32), rng.uniform(0, 1, (16, 16, 2)).astype(F32))
    c2w = torch.from_numpy(f["c2ws_p"][:1])
    mvp = torch.matmul(camera.intr_to_proj(torch.from_numpy(f["intr_p"]), perspective=True), camera.c2w_to_w2c(c2w)).cuda().contiguous()
    verts, faces = _cu(f["verts"]), _cu(f["faces"], torch.int32)
    clip, _ = ops.transform_points(verts, mvp, want_ndc=False)
    rast = ops.rasterize(clip[0].contiguous(), faces, size, size)
    kd = _cu(np.ascontiguousarray(f["tex"][:, :, :3]).astype(F32) / F32(255.0))
    tng = meshes.vertex_tangents(f["verts"], f["faces"], f["uvs"], f["v_nrm"])
    fn = ops.face_normals(verts, faces)
    args = (rast, faces, verts, _cu(f["v_nrm"]), _cu(f["uvs"]), kd, None, c2w[0, :3, 3].tolist(), _cu(ld), _cu(ls), _cu(lut))
    return f, args, tng, fn, c2w[0, :3, 3].numpy()


def test_flat_map_on_a_torus_frame():
    """a flat map (0.5, 0.5, 1) gives p = (0, 0, 1): s = normalize(sn).  Where the face looks at the eye and dot(vv, sn) >= 0.1 the blend weight is 1 and the
    frame is the no-map frame up to the shading normal's own bound (p.y = 0, r = 1: ds = 45 u, and dt where dot / 0.1 is within dt of 1) propagated through
    the lookups (lights of 8^2 faces in [0, 2), a 16^2 table), plus 2 ulp of the maximum for the sum of the two terms."""
    from unitex_amd.texturetools import ops
    f, args, tng, fn, eye = _torus_frame()
    flat = _cu(np.broadcast_to(np.array([0.5, 0.5, 1.0], F32), (4, 4, 3)).copy())
    nm = dict(v_tng=tng.cuda(), f_nrm=fn, bg=(0.25, 0.5, 0.75), want_rgba=True)
    u8, rgba = ops.pbr_shade(*args, normal_map=flat, **nm)
    u8b, rgbab = ops.pbr_shade(*args, normal_map=flat, **nm)
    assert np.array_equal(u8.cpu().numpy(), u8b.cpu().numpy()) and np.array_equal(rgba.cpu().numpy(), rgbab.cpu().numpy()), "run-to-run identical"
    _, plain = ops.pbr_shade(*args, bg=(0.25, 0.5, 0.75), want_rgba=True)
    rgba, plain = rgba.cpu().numpy(), plain.cpu().numpy()
    assert np.isfinite(rgba).all()
    # the dense inputs of every covered pixel, fp64 on the host
    rast = args[0].cpu().numpy().astype(np.float64)
    cov = rast[..., 3] > 0
    tri = f["faces"][np.maximum(rast[..., 3].astype(np.int64) - 1, 0)]
    u, v = rast[..., 0:1], rast[..., 1:2]
    interp = lambda a: a[tri[..., 0]].astype(np.float64) * u + a[tri[..., 1]].astype(np.float64) * v + a[tri[..., 2]].astype(np.float64) * (1 - u - v)
    g = fn.cpu().numpy()[np.maximum(rast[..., 3].astype(np.int64) - 1, 0)]
    p = np.broadcast_to(np.array([0.0, 0.0, 1.0]), g.shape)
    out, parts = PC.shading_normal(eye, interp(f["verts"]), p, interp(f["v_nrm"]), interp(tng.numpy()), g, parts=True)
    vv = PC.unit(eye.astype(np.float64) - interp(f["verts"]))
    sel = cov & (parts["gdot"] > 0) & ((vv * PC.unit(interp(f["v_nrm"]))).sum(-1) >= 0.1)
    assert sel.sum() > 200 and (cov & ~sel).any(), "both kinds of pixel are in the frame"
    bd, bs = PC.shade_bounds(PC.shading_normal_bound(parts), out, 8, 2.0, 2.0, 16)
    bound = bd + bs + 2 * _ulp(plain[cov][:, :3])
    e = np.abs(rgba[..., :3] - plain[..., :3]).max(-1)
    print("flat map vs no map on %d pixels: max %.3g (%.3g of the bound); elsewhere max %.3g" % (sel.sum(), e[sel].max(), (e[sel] / bound[sel]).max(), e[cov & ~sel].max()))
    assert (e[sel] <= bound[sel]).all()
    assert np.array_equal(rgba[~cov], plain[~cov]) and np.array_equal(rgba[..., 3], plain[..., 3])
    tilted = _cu(np.broadcast_to(np.array([0.8, 0.35, 0.75], F32), (4, 4, 3)).copy())
    _, rt = ops.pbr_shade(*args, normal_map=tilted, **nm)
    assert np.abs(rt.cpu().numpy()[sel][:, :3] - rgba[sel][:, :3]).max() > 1e-2, "a tilted map changes the frame"


def test_export_orbit_video_with_a_normal_map(tmp_path):
    from unitex_amd.texturetools import camera, meshes, ops
    from unitex_amd.texturetools.pbr import PBRModel
    from unitex_amd.texturetools.renderer_inverse import TexturedMesh
    from unitex_amd.texturetools.video import VideoExporter, _vertex_normals
    f = _torus()
    verts = meshes.normalise_to_bbox(f["verts"], 1.0)
    assert np.array_equal(meshes.normalise_to_bbox(verts, 1.0), verts), "the .glb path rescales to the bbox: a fixed point keeps both routes on the same vertices"
    uvs = (np.round(f["uvs"] * 256) / 256).astype(F32)          # 1 - v is exact, so the glTF's top-down v reads back bit for bit
    rng = np.random.default_rng(4)
    tex = f["tex"][:, :, :3]
    bump = rng.integers(0, 256, tex.shape[:2] + (3,)).astype(np.uint8)
    bump[..., 2] = 128 + bump[..., 2] // 2
    mr = np.zeros_like(tex)
    mr[..., 0], mr[..., 1] = 255, 255          # the constant [1, 1, 0] at Kd's size: bit-identical to the default a path is shaded with (its Ks is not read)
    mesh = TexturedMesh(verts, f["faces"], uvs, tex, metallic_roughness=mr, bump=bump)
    model = PBRModel(np.random.default_rng(2).uniform(0, 2, (8, 16, 3)).astype(F32), device="cuda:0", cube_res=16, roughness=0.5)
    ex = VideoExporter(device="cuda:0")
    kw = dict(n_frames=2, render_size=64, return_frames=True, pbr_model=model)
    lit = ex.export_orbit_video(mesh, str(tmp_path / "a.mp4"), normal_map=True, **kw)
    assert len(lit) == 2 and lit[0].shape == (64, 64, 3) and lit[0].dtype == np.uint8
    # the same frames from per-frame ops.pbr_shade calls
    c2ws = camera.generate_orbit_views_c2ws(3, radius=2.8, height=0.0, theta_0=0.0, degree=True)[:2]
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    mvp = torch.matmul(camera.intr_to_proj(intr, perspective=True), camera.c2w_to_w2c(c2ws)).cuda().contiguous()
    vd, fd = _cu(verts), _cu(f["faces"], torch.int32)
    nrm = _vertex_normals(torch.from_numpy(verts), torch.from_numpy(f["faces"]), ex.normal_weighting)
    to_tex = lambda a: _cu(np.ascontiguousarray(a[::-1]).astype(F32) / F32(255.0))
    clip, _ = ops.transform_points(vd, mvp, want_ndc=False)
    for i in range(2):
        rast = ops.rasterize(clip[i].contiguous(), fd, 64, 64)
        want = ops.pbr_shade(rast, fd, vd, nrm.cuda(), _cu(uvs), to_tex(tex), to_tex(mr), c2ws[i, :3, 3].tolist(), model.light_diffuse, model.light_specular,
                             model.FG_LUT[0], v_tng=meshes.vertex_tangents(verts, f["faces"], uvs, nrm).cuda(), f_nrm=ops.face_normals(vd, fd), normal_map=to_tex(bump))
        assert np.array_equal(want.cpu().numpy(), lit[i])
    # the exported .glb, read back from its path (normalTexture; its Ks is the default [1, 1, 0], which is what `mr` holds)
    glb = str(tmp_path / "m.glb")
    mesh.export(glb)
    assert np.array_equal(meshes.load_material_textures(glb)["normal"], bump)
    from_path = ex.export_orbit_video(glb, str(tmp_path / "b.mp4"), normal_map=True, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(lit, from_path))
    as_tuple = ex.export_orbit_video((verts, f["faces"], uvs, tex, None, mr, bump), str(tmp_path / "c.mp4"), normal_map=True, **kw)
    as_array = ex.export_orbit_video((verts, f["faces"], uvs, tex, None, mr), str(tmp_path / "d.mp4"), normal_map=bump, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(lit, as_tuple)) and all(np.array_equal(a, b) for a, b in zip(lit, as_array))
    unlit_normal = ex.export_orbit_video(mesh, str(tmp_path / "e.mp4"), normal_map=None, **kw)
    assert not np.array_equal(unlit_normal[0], lit[0])
    assert all(np.array_equal(a, b) for a, b in zip(unlit_normal, ex.export_orbit_video(mesh, str(tmp_path / "f.mp4"), **kw))), "None is the call without the argument"
    with pytest.raises(ValueError):          # no map on the mesh
        ex.export_orbit_video((verts, f["faces"], uvs, tex), str(tmp_path / "g.mp4"), normal_map=True, **kw)
    with pytest.raises(ValueError):          # no model
        ex.export_orbit_video(mesh, str(tmp_path / "h.mp4"), n_frames=2, render_size=64, normal_map=True)
    obj = str(tmp_path / "m.obj")
    mesh.export(obj)
    with pytest.raises(ValueError):          # a path that is no .glb
        ex.export_orbit_video(obj, str(tmp_path / "i.mp4"), normal_map=True, **kw)


def test_degenerate_inputs_stay_finite():
    """8 x 8 pixels (npix = 64, a quarter of a block), one launch of each entry: zero tangents, tangents parallel to the normals, a zero map (p = -1: p.z clamps
    to 0), a zero perturbation (0.5) and zero geometric normals"""
    from unitex_amd.texturetools import ops
    S = 8
    g = ((np.arange(S) + 0.5) / S).astype(F32)
    yy, xx = np.meshgrid(g, g, indexing="ij")
    lower = xx >= yy
    rast = np.zeros((S, S, 4), F32)
    rast[..., 0], rast[..., 1] = np.where(lower, 1 - xx, 1 - yy), np.where(lower, xx - yy, xx)
    rast[..., 2], rast[..., 3] = 0.5, np.where(lower, 1.0, 2.0)
    rast[0, :, 3] = 0.0
    verts = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0.2], [-1, 1, 0]], F32)
    nrm = np.array([[0, 0, 1], [0, 0, 2], [0.2, 0, 1], [0, 0, 1]], F32)
    tng = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 3]], F32)          # triangle 0: zero tangents; triangle 1 blends zero with one parallel to the normal
    uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    fnrm = np.array([[0, 0, 1], [0, 0, 0]], F32)
    nm = np.zeros((S, S, 3), F32)
    nm[2:4], nm[4:6], nm[6:] = 0.5, np.array([0.5, 0.5, 0.0], F32), np.random.default_rng(1).uniform(0, 1, (2, S, 3)).astype(F32)
    rng = np.random.default_rng(3)
    ld, ls, lut = (_cu(rng.uniform(0, 2, (6, 8, 8, 3)).astype(F32)), _cu(rng.uniform(0, 2, (6, 8, 8, 3)).astype(F32)), _cu(rng.uniform(0, 1, (16, 16, 2)).astype(F32)))
    kd = _cu(rng.uniform(0, 1, (S, S, 3)).astype(F32))
    u8, rgba = ops.pbr_shade(_cu(rast), _cu(faces), _cu(verts), _cu(nrm), _cu(uvs), kd, None, [0.3, -0.2, 2.5], ld, ls, lut, bg=(1.0, 0.5, 0.0), want_rgba=True,
                             v_tng=_cu(tng), f_nrm=_cu(fnrm), normal_map=_cu(nm))
    rgba = rgba.cpu().numpy()
    assert np.isfinite(rgba).all() and (rgba[0, :, :3] == np.array([1.0, 0.5, 0.0], F32)).all() and (rgba[1:, :, 3] == 1).all()
    z = np.zeros((S * S, 3), F32)
    pos = rng.uniform(-1, 1, (S * S, 3)).astype(F32)
    n = rng.uniform(-1, 1, (S * S, 3)).astype(F32)
    p = rng.uniform(-1, 1, (S * S, 3)).astype(F32)
    t = rng.uniform(-1, 1, (S * S, 3)).astype(F32)
    t[:16], t[16:32] = 0.0, n[16:32] * F32(-2.0)
    p[8:24], p[32:40] = 0.0, np.array([0.0, 0.0, -1.0], F32)
    n[40:44], gn = 0.0, n.copy()
    gn[44:48] = 0.0
    out = ops.pbr_shading_normal(_cu(np.array([0.1, 0.2, 3.0], F32)), _cu(pos), _cu(p), _cu(n), _cu(t), _cu(gn)).cpu().numpy()
    want = PC.shading_normal(np.array([0.1, 0.2, 3.0], F32), pos, p, n, t, gn)
    assert np.isfinite(out).all() and np.isfinite(want).all()
    exact = np.r_[8:16, 32:40]          # s = 0 exactly (zero tangent with zero p; p = (0, 0, -1)): out = +-g
    front = ((gn.astype(np.float64) * PC.unit(np.array([0.1, 0.2, 3.0], F32).astype(np.float64) - pos)).sum(-1) > 0)[:, None]
    assert np.array_equal(out[exact], np.where(front, gn, -gn)[exact])
    assert ops.pbr_shading_normal(_cu(z[0]), _cu(z), _cu(z), _cu(z), _cu(z), _cu(z)).abs().max().item() == 0.0
