"""Atlas-space view projection and face / vertex visibility on the GPU: utx_visible_faces_rays / _raster, utx_erode_faces, utx_visible_vertices,
utx_uv_project, their ops wrappers and the public methods of NVDiffRendererInverse against the reference's own results (fixture G19), the numpy
restatement (oracle/uv_project_ref.py), the composition of the existing ops, a float64 brute-force ray caster, and at the edges.
Standards: the docstring of tests/test_uv_project_cpu.py -- masks, uv_alpha, uv, 'nearest' / 'nvdiffrast' map_attr and every background form
bit-exact on the fixture's own v_ndc and rasters; 'bilinear' map_attr within MAP_BOUND.  The kernel is bit-identical to the restatement in all
three filters (asserted here), so its deviation from G19 is the restatement's.
End to end the per-vertex NDC is this build's own (utx_transform_points in place of torch.matmul and a division), so the public method is held
bit-exactly to the restatement fed with the build's own v_ndc and rasters, its face masks exactly to G19, and its uv to G19 within E2E_UV: with
S = sum_j |m_ij| |v_j| of the clip rows (float64), a float32 row product in any order is within 4 u S of the exact one (four products, three
additions), so x / w is within (4 u S_x + |ndc| 4 u S_w) / |w| + u |ndc| on each side; twice that for the two sides, carried through the
interpolation (a convex combination, plus 3 u max|ndc| of its own rounding on each side)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import uv_project_ref as R

pytestmark = pytest.mark.gpu
F32, F64, U = np.float32, np.float64, 2.0 ** -24
SENTINEL = 0x5A


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _faces(f):
    return _cu(f["faces"], torch.int32)


def _project(f, tag, mask, m=None, i=0, mode="bilinear", bg=None):
    from unitex_amd.texturetools import ops
    if isinstance(bg, np.ndarray):
        bg = float(bg) if bg.ndim == 0 else _cu(bg)
    out = ops.uv_project(_cu(f["rast2d"]), _faces(f), _cu(mask, torch.uint8), _cu(f["v_ndc_" + tag]), None if m is None else _cu(m),
                         None if m is None else _cu(f["rast_map_%d_%s" % (i, tag)]), filter=mode, background=bg)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bvh(verts, faces):
    from unitex_amd.texturetools import ops
    return ops.BVH(_cu(verts), _cu(faces, torch.int32))


@pytest.mark.parametrize("tag,perspective", R.SETS)
def test_ops_against_g19(tag, perspective):
    from unitex_amd.texturetools import ops
    f = R.load()
    Fn, V = f["faces"].shape[0], f["verts"].shape[0]
    bvh = _bvh(f["verts"], f["faces"])
    rays = ops.visible_faces_rays(bvh, _cu(f["c2ws_" + tag]), perspective=perspective)
    assert rays.dtype == torch.uint8 and np.array_equal(rays.cpu().numpy(), f["faces_rays_e0_" + tag])
    for kw in (dict(force_stack=True), dict(face_order=True), dict(force_stack=True, face_order=True)):
        assert torch.equal(ops.visible_faces_rays(bvh, _cu(f["c2ws_" + tag]), perspective=perspective, **kw), rays), kw
    assert np.array_equal(ops.erode_faces(rays, _faces(f), V, 1).cpu().numpy(), f["faces_rays_e1_" + tag])
    assert np.array_equal(ops.visible_vertices(rays, _faces(f), V).cpu().numpy(), f["verts_rays_e0_" + tag])
    rast = ops.visible_faces_raster(_cu(f["rast_view_" + tag]), Fn)
    assert np.array_equal(rast.cpu().numpy(), f["faces_raster_e0_" + tag])
    for e in (0, 1):
        m = ops.erode_faces(rast, _faces(f), V, e)
        assert np.array_equal(m.cpu().numpy(), f["faces_raster_e%d_%s" % (e, tag)])
        assert np.array_equal(ops.visible_vertices(m, _faces(f), V).cpu().numpy(), f["verts_raster_e%d_%s" % (e, tag)])
    mask = f["faces_rays_e0_" + tag]
    got = _project(f, tag, mask)
    assert sorted(got) == ["uv", "uv_alpha"]
    assert got["uv"].tobytes() == f["uv_" + tag].tobytes() and got["uv_alpha"].tobytes() == f["uv_alpha_" + tag].tobytes()
    worst = 0.0
    for key, m, i, mode, bg in R.cases(f, tag):
        got = _project(f, tag, mask, m, i, mode, bg)
        assert got["uv"].tobytes() == f["uv_" + tag].tobytes() and got["uv_alpha"].tobytes() == f["uv_alpha_map_%d_%s" % (i, tag)].tobytes(), key
        dev = R.check_map(key, got["map_attr"], f[key], mode, m)
        worst = max(worst, dev if mode == "bilinear" else 0.0)
        ref = R.uv_project(f["rast2d"], f["faces"], mask, f["v_ndc_" + tag], m, f["rast_map_%d_%s" % (i, tag)], mode, bg)
        assert got["map_attr"].tobytes() == ref["map_attr"].tobytes(), "%s: the kernel is not the restatement" % key
    print("bilinear map_attr of utx_uv_project against G19, set %s: at most %.2f u" % (tag, worst))


def _e2e_uv_bound(f, tag, perspective):
    from unitex_amd.texturetools import camera
    c2ws, intr = torch.from_numpy(f["c2ws_" + tag].copy()), torch.from_numpy(f["intr_" + tag].copy())
    mvp = torch.matmul(camera.intr_to_proj(intr, perspective=perspective), camera.c2w_to_w2c(c2ws)).numpy().astype(F64)
    vh = np.concatenate([f["verts"].astype(F64), np.ones((f["verts"].shape[0], 1))], 1)
    S = np.einsum("bij,vj->bvi", np.abs(mvp), np.abs(vh))
    clip = np.einsum("bij,vj->bvi", mvp, vh)
    ndc = np.abs(clip[..., :2] / clip[..., 3:4])
    per_vertex = (4 * U * S[..., :2] + ndc * 4 * U * S[..., 3:4]) / np.abs(clip[..., 3:4]) + U * ndc
    return 2.0 * (per_vertex.max() + 3 * U * ndc.max())


@pytest.mark.parametrize("tag,perspective", R.SETS)
def test_public_methods_against_g19(tag, perspective):
    from unitex_amd.texturetools import ops
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    f = R.load()
    inv = NVDiffRendererInverse(device="cuda:0").update_from_arrays(f["verts"], f["faces"], f["uvs"])
    c2ws, intr = torch.from_numpy(f["c2ws_" + tag].copy()), torch.from_numpy(f["intr_" + tag].copy())
    for e in (0, 1):
        m = inv.get_visible_faces(c2ws, perspective=perspective, erode_neighbor=e)
        assert m.dtype == torch.bool and np.array_equal(m.cpu().numpy(), f["faces_rays_e%d_%s" % (e, tag)] > 0)
    assert np.array_equal(inv.get_visible_vertices(c2ws, perspective=perspective).cpu().numpy(), f["verts_rays_e0_" + tag] > 0)
    # the raster method runs this build's rasteriser on this build's clip coordinates: held to the restatement on the method's own raster
    rast = inv._view_raster(c2ws, intr, R.RASTER_SIZE, perspective)[4]
    for e in (0, 1, 2):
        want = R.erode_faces(R.visible_faces_raster(rast.cpu().numpy(), f["faces"].shape[0]), f["faces"], f["verts"].shape[0], e)
        got = inv.get_visible_faces(c2ws, perspective=perspective, method="raster", intrinsics=intr, render_size=R.RASTER_SIZE, erode_neighbor=e)
        assert np.array_equal(got.cpu().numpy(), want)
        gotv = inv.get_visible_vertices(c2ws, perspective=perspective, method="raster", intrinsics=intr, render_size=R.RASTER_SIZE, erode_neighbor=e)
        assert np.array_equal(gotv.cpu().numpy(), R.visible_vertices(want, f["faces"], f["verts"].shape[0]))
    bound = _e2e_uv_bound(f, tag, perspective)
    m = f["map_0"]
    out = inv.simple_inverse_rendering(c2ws, R.ATLAS, intrinsics=intr, perspective=perspective, map_attr=torch.from_numpy(m.copy()), render_uv=True,
                                       render_map_attr=True, grid_interpolate_mode="nearest", enable_antialis=False)
    assert sorted(out) == ["alpha", "map_attr", "mask", "uv", "uv_alpha"] and out["map_attr"].shape == (R.B,) + R.ATLAS + (3,)
    alone = inv.simple_inverse_rendering(c2ws, R.ATLAS, intrinsics=intr, perspective=perspective, render_uv=True)
    assert alone["uv_alpha"].cpu().numpy().tobytes() == f["uv_alpha_" + tag].tobytes()
    d = np.abs(alone["uv"].cpu().numpy().astype(F64) - f["uv_" + tag].astype(F64)).max()
    print("uv of the public method against G19, set %s: max|diff| %.3g = %.2f u (bound %.2f u)" % (tag, d, d / U, bound / U))
    assert d <= bound and torch.equal(alone["uv"], out["uv"])
    # bit-exact against the restatement on the build's own v_ndc and rasters
    ndc, rast_map = inv._view_raster(c2ws, intr, m.shape[1:3], perspective)[3:5]
    ref = R.uv_project(f["rast2d"], f["faces"], f["faces_rays_e0_" + tag], ndc.cpu().numpy(), m, rast_map.cpu().numpy(), "nearest", None)
    for k in ("uv", "uv_alpha", "map_attr"):
        assert out[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
    # render_uv together with the camera-dependent flags equals the separate calls (the reference raises TypeError there, G19)
    both = inv.simple_inverse_rendering(c2ws, R.ATLAS, intrinsics=intr, perspective=perspective, render_uv=True, render_camera_position=True,
                                        render_distance=True, render_cos_ray_normal=True)
    geo = inv.simple_inverse_rendering(c2ws, R.ATLAS, render_camera_position=True, render_distance=True, render_cos_ray_normal=True)
    for k in geo:
        assert torch.equal(both[k], geo[k]), k
    assert torch.equal(both["uv"], alone["uv"]) and torch.equal(both["uv_alpha"], alone["uv_alpha"])
    # the raster method of simple_inverse_rendering takes its size from the map
    ras = inv.simple_inverse_rendering(c2ws, R.ATLAS, intrinsics=intr, perspective=perspective, map_attr=torch.from_numpy(m.copy()), render_uv=True,
                                       render_map_attr=True, visible_faces="raster", background=0.5)
    fm = R.visible_faces_raster(rast_map.cpu().numpy(), f["faces"].shape[0])
    ref = R.uv_project(f["rast2d"], f["faces"], fm, ndc.cpu().numpy(), m, rast_map.cpu().numpy(), "bilinear", F32(0.5))
    for k in ("uv", "uv_alpha", "map_attr"):
        assert ras[k].cpu().numpy().tobytes() == ref[k].tobytes(), k


def test_sentinels_around_every_output():
    """every output buffer sits between guard bytes that the launch must leave alone (the raw entry points, caller-owned memory)"""
    from unitex_amd.flux.ops import get_ctx
    from unitex_amd._lib import ptr
    f = R.load()
    tag, Fn, V = "p", f["faces"].shape[0], f["verts"].shape[0]
    H, W = R.ATLAS
    ctx = get_ctx(0)
    G = 256

    def guarded(nbytes):
        t = torch.full((nbytes + 2 * G,), SENTINEL, dtype=torch.uint8, device="cuda")
        return t, t[G:G + nbytes]

    def intact(t, nbytes):
        return bool((t[:G] == SENTINEL).all()) and bool((t[G + nbytes:] == SENTINEL).all())
    bvh = _bvh(f["verts"], f["faces"])
    faces, c2ws = _faces(f), _cu(f["c2ws_" + tag])
    t_mask, mask = guarded(R.B * Fn)
    ctx.check(ctx.lib.utx_visible_faces_rays(ctx.handle, bvh.handle, ptr(bvh.verts), ptr(bvh.faces), Fn, ptr(c2ws), R.B, 1, 0, ptr(mask), None, ctx.stream()))
    assert intact(t_mask, R.B * Fn) and np.array_equal(mask.cpu().numpy().reshape(R.B, Fn), f["faces_rays_e0_" + tag])
    t_v, vout = guarded(R.B * V)
    ctx.check(ctx.lib.utx_visible_vertices(ctx.handle, ptr(mask), ptr(faces), R.B, Fn, V, ptr(vout), ctx.stream()))
    assert intact(t_v, R.B * V) and np.array_equal(vout.cpu().numpy().reshape(R.B, V), f["verts_rays_e0_" + tag])
    t_s, stamp = guarded(R.B * V * 4)
    ctx.check(ctx.lib.utx_erode_faces(ctx.handle, ptr(mask), ptr(faces), R.B, Fn, V, 1, ptr(stamp), ctx.stream()))
    assert intact(t_s, R.B * V * 4) and intact(t_mask, R.B * Fn) and np.array_equal(mask.cpu().numpy().reshape(R.B, Fn), f["faces_rays_e1_" + tag])
    t_r, rmask = guarded(R.B * Fn)
    rv = _cu(f["rast_view_" + tag])
    ctx.check(ctx.lib.utx_visible_faces_raster(ctx.handle, ptr(rv), R.B, rv.shape[1], rv.shape[2], Fn, ptr(rmask), ctx.stream()))
    assert intact(t_r, R.B * Fn) and np.array_equal(rmask.cpu().numpy().reshape(R.B, Fn), f["faces_raster_e0_" + tag])
    m = _cu(f["map_1"])
    n = R.B * H * W
    (t_uv, uv), (t_a, alpha), (t_m, mo) = guarded(n * 2 * 4), guarded(n * 4), guarded(n * 5 * 4)
    fm, rast2d, ndc, rast_map = _cu(f["faces_rays_e0_" + tag]), _cu(f["rast2d"]), _cu(f["v_ndc_" + tag]), _cu(f["rast_map_1_" + tag])      # held until the launch has run
    ctx.check(ctx.lib.utx_uv_project(ctx.handle, ptr(rast2d), ptr(faces), Fn, ptr(fm), ptr(ndc), V, R.B, H, W, ptr(m), R.B, 8, 8, 5,
                                     ptr(rast_map), 2, 0, 0.0, None, ptr(uv), ptr(alpha), ptr(mo), ctx.stream()))
    assert intact(t_uv, n * 8) and intact(t_a, n * 4) and intact(t_m, n * 20)
    assert uv.cpu().numpy().tobytes() == f["uv_" + tag].tobytes() and mo.cpu().numpy().tobytes() == f["map_1_b_nvdiffrast_" + tag].tobytes()
    assert alpha.cpu().numpy().tobytes() == f["uv_alpha_map_1_" + tag].tobytes()


def _synthetic(f, B, rng):
    """a v_ndc of the test's own on the atlas of G19: coordinates beyond +-1 (taps outside the map in every filter) and, on two faces, exact quarters
    (texels on an exact half of the 8-wide and 24-wide maps, where 'nearest' rounds to even); a random face mask and random view coverage"""
    V, Fn = f["verts"].shape[0], f["faces"].shape[0]
    v_ndc = rng.uniform(-1.3, 1.3, (B, V, 2)).astype(F32)
    v_ndc[:, f["faces"][5]] = F32(-0.75)
    v_ndc[:, f["faces"][70]] = F32(0.25)
    mask = (rng.uniform(size=(B, Fn)) < 0.7).astype(np.uint8)
    mask[:, [5, 70]] = 1
    return v_ndc, mask


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("Bm,C_", ((1, 3), (3, 5), (1, 1)))
def test_composition_of_existing_ops(mode, Bm, C_):
    """utx_uv_project is bit-identical to ops.interpolate + the map lookup of ops.screen_gbuffer (the map and, in 'nearest', the view's coverage) +
    torch indexing, for every filter and background form; the rasters of the coverage come from ops.rasterize"""
    from unitex_amd.texturetools import ops
    f = R.load()
    B, (H, W) = 3, R.ATLAS
    rng = np.random.default_rng(190 + C_)
    v_ndc, mask = _synthetic(f, B, rng)
    Hm, Wm = (8, 8) if C_ == 5 else (16, 24)
    m = _cu(rng.uniform(0, 1, (Bm, Hm, Wm, C_)).astype(F32))
    faces, rast2d, ndc_t, mask_t = _faces(f), _cu(f["rast2d"]), _cu(v_ndc), _cu(mask)
    clip = _cu(np.concatenate([f["v_ndc_p"] * F32(1.6), np.zeros((B, v_ndc.shape[1], 1), F32), np.ones((B, v_ndc.shape[1], 1), F32)], -1))
    rast_map = torch.stack([ops.rasterize(clip[b].contiguous(), faces, Hm, Wm) for b in range(B)])
    tri = rast2d[..., 3].long() - 1
    vis = (tri >= 0)[None] & (mask_t[:, tri.clamp(min=0)] != 0)
    rast_vis = torch.cat([rast2d[None, ..., :3].expand(B, -1, -1, -1), torch.where(vis, rast2d[..., 3][None], 0.0)[..., None]], -1).contiguous()
    uv = torch.stack([torch.where(vis[b][..., None], ops.interpolate(ndc_t[b].contiguous(), rast_vis[b], faces), -1.0) for b in range(B)])
    s, cov = [], []
    for b in range(B):
        kw = dict(v_uv=ndc_t[b].contiguous(), want=("map_attr",))
        s.append(ops.screen_gbuffer(rast_vis[b:b + 1], faces, _cu(f["verts"]), maps=(m[b if Bm > 1 else 0],), filter=mode, **kw)["map_attr"][0])
        covmap = (rast_map[b, ..., 3:4] > 0).float().contiguous()
        cov.append(ops.screen_gbuffer(rast_vis[b:b + 1], faces, _cu(f["verts"]), maps=(covmap,), filter="nearest", **kw)["map_attr"][0, ..., 0] >= 1)
    s, cov = torch.stack(s), torch.stack(cov)
    assert bool((vis & ~cov).any()) and bool((vis & cov).any())
    alpha = vis & cov
    dense = _cu(rng.uniform(0, 1, (B, H, W, C_)).astype(F32))
    for bg in (None, 0.25, dense[0, 0, 0].contiguous(), dense):
        got = ops.uv_project(rast2d, faces, mask_t, ndc_t, m, rast_map, filter=mode, background=bg)
        if bg is None:
            want = torch.where(cov[..., None], s, m[:, 0, 0][:, None, None, :].expand(B, 1, 1, C_))
        else:
            want = torch.where(alpha[..., None], s, bg if isinstance(bg, torch.Tensor) else torch.full_like(s, bg))
        assert torch.equal(got["uv"], uv) and torch.equal(got["uv_alpha"][..., 0], alpha.float())
        assert got["map_attr"].cpu().numpy().tobytes() == want.contiguous().cpu().numpy().tobytes(), (mode, Bm, C_, type(bg))
    # the conditions the synthetic v_ndc is there for
    uvn, visn = uv.cpu().numpy(), vis.cpu().numpy()
    ix = ((uvn[..., 0] + F32(1)) * F32(Wm) - F32(1)) * F32(0.5)
    assert (visn & ((np.floor(ix) < 0) | (np.floor(ix) + 1 >= Wm))).any(), "no visible texel with a tap outside the map"
    assert (visn & (ix - np.floor(ix) == 0.5) & (np.floor(ix) % 2 == 0)).any(), "no visible texel on an exact half below an even index"


def _two_spheres(n_lat=12, n_lon=16):
    """two UV spheres of n_lat x n_lon segments, the second smaller and offset so that each hides part of the other from most directions"""
    def sphere(c, r, phase):
        v, fa = [], []
        for i in range(n_lat + 1):
            th = np.pi * i / n_lat
            for j in range(n_lon):
                ph = 2 * np.pi * j / n_lon + phase
                v.append([c[0] + r * np.sin(th) * np.cos(ph), c[1] + r * np.cos(th), c[2] + r * np.sin(th) * np.sin(ph)])
        idx = lambda i, j: i * n_lon + j % n_lon
        for i in range(n_lat):
            for j in range(n_lon):
                if i > 0:
                    fa.append([idx(i, j), idx(i + 1, j), idx(i, j + 1)])
                if i < n_lat - 1:
                    fa.append([idx(i, j + 1), idx(i + 1, j), idx(i + 1, j + 1)])
        return np.array(v), np.array(fa)
    v0, f0 = sphere((-0.31, 0.07, 0.11), 0.62, 0.013)
    v1, f1 = sphere((0.47, -0.13, -0.23), 0.41, 0.291)
    return np.concatenate([v0, v1]).astype(F32), np.concatenate([f0, f1 + len(v0)]).astype(np.int32)


def _orbit(angles_deg, radius=2.9, height=0.6):
    """c2w of cameras on a ring, looking at the origin (column 2 points from the target to the camera, as in the reference's c2w)"""
    out = []
    for a in np.deg2rad(angles_deg):
        eye = np.array([radius * np.sin(a), height, radius * np.cos(a)])
        z = eye / np.linalg.norm(eye)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
        out.append(m)
    return np.array(out, F32)


@pytest.mark.parametrize("perspective", (True, False))
def test_ray_visibility_against_float64_brute_force(perspective):
    from unitex_amd.texturetools import ops
    verts, faces = _two_spheres()
    c2ws = _orbit((17.0, 101.0, 233.0))
    ref, must_set, may_differ, share = R.decided_faces(verts, faces, c2ws, perspective)
    hit = R.visible_faces_rays(verts, faces, c2ws, perspective)[1]
    print("two spheres, F = %d: %.3f %% of the rays fail the margin (float64 alone); %d of %d faces are left to them" %
          (faces.shape[0], 100 * share, int(may_differ.sum()), may_differ.size))
    assert share <= 0.01
    bvh = _bvh(verts, faces)
    got, nodes = ops.visible_faces_rays(bvh, _cu(c2ws), perspective=perspective, count=True)
    got = got.cpu().numpy() > 0
    # every face is compared exactly, except those a margin-failing ray could hit first (R.decided_faces): a face that a margin-passing ray hits
    # must be marked, and outside the reach of the failing rays the mask is the reference's
    assert R.mask_agrees(got, ref, must_set, may_differ) is None, R.mask_agrees(got, ref, must_set, may_differ)
    other = ops.visible_faces_rays(bvh, _cu(c2ws), perspective=perspective, face_order=True, count=True)
    stack = ops.visible_faces_rays(bvh, _cu(c2ws), perspective=perspective, force_stack=True)
    assert np.array_equal(other[0].cpu().numpy() > 0, got) and np.array_equal(stack.cpu().numpy() > 0, got)
    print("nodes visited per ray: %.1f in the tree's leaf order, %.1f in face order" % (nodes / ref.size, other[1] / ref.size))
    assert not ref.all(1).any() and ((hit != np.arange(faces.shape[0])[None]) & (hit >= 0)).any()


@pytest.mark.parametrize("Fn", (1, 255, 256, 257))
@pytest.mark.parametrize("B", (1, 3))
def test_edges_of_the_launch_geometry(Fn, B):
    """F around the block size, B = 1 and 3, the packed and the stack walk, both ray orders; erosion at depth 0, 1 and 2 and the vertex masks against
    the restatement; the projection on a 1 x 1 atlas"""
    from unitex_amd.texturetools import ops
    verts, faces = _two_spheres()
    faces = np.ascontiguousarray(faces[np.linspace(0, faces.shape[0] - 1, Fn).astype(np.int64)])
    V = verts.shape[0]
    c2ws = _orbit((17.0, 101.0, 233.0))[:B]
    ref, must_set, may_differ, _ = R.decided_faces(verts, faces, c2ws, True)
    assert may_differ.sum() <= 0.05 * may_differ.size and must_set.any(1).all() and not ref.all(1).any() or Fn == 1
    bvh = _bvh(verts, faces)
    got = ops.visible_faces_rays(bvh, _cu(c2ws))
    assert got.shape == (B, Fn)
    # against the float64 brute force, face by face, at every size: exact outside the reach of the few margin-failing rays (R.decided_faces)
    assert R.mask_agrees(got.cpu().numpy() > 0, ref, must_set, may_differ) is None, R.mask_agrees(got.cpu().numpy() > 0, ref, must_set, may_differ)
    for kw in (dict(force_stack=True), dict(face_order=True), dict(force_stack=True, face_order=True)):
        assert torch.equal(ops.visible_faces_rays(bvh, _cu(c2ws), **kw), got)
    ft = _cu(faces, torch.int32)
    for depth in (0, 1, 2):
        e = ops.erode_faces(got, ft, V, depth)
        assert np.array_equal(e.cpu().numpy() > 0, R.erode_faces(got.cpu().numpy(), faces, V, depth))
        assert np.array_equal(ops.visible_vertices(e, ft, V).cpu().numpy() > 0, R.visible_vertices(e.cpu().numpy(), faces, V))
    # a 1 x 1 atlas whose texel lies in face Fn - 1
    rast2d = np.array([[[0.25, 0.5, 0.0, Fn]]], F32)
    rng = np.random.default_rng(Fn + B)
    v_ndc = rng.uniform(-1, 1, (B, V, 2)).astype(F32)
    m = rng.uniform(0, 1, (B, 4, 6, 3)).astype(F32)
    rast_map = np.zeros((B, 4, 6, 4), F32)
    rast_map[..., 3] = rng.integers(0, 2, (B, 4, 6))
    out = ops.uv_project(_cu(rast2d), ft, got, _cu(v_ndc), _cu(m), _cu(rast_map), filter="nearest", background=None)
    want = R.uv_project(rast2d, faces, got.cpu().numpy(), v_ndc, m, rast_map, "nearest", None)
    for k in ("uv", "uv_alpha", "map_attr"):
        assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k


def test_error_codes_on_the_device():
    """the checks that need a live tree: a tree of another F; and the argument checks with real device memory behind the pointers"""
    from unitex_amd.flux.ops import get_ctx
    from unitex_amd._lib import ptr
    f = R.load()
    ctx = get_ctx(0)
    bvh = _bvh(f["verts"], f["faces"])
    Fn, V = f["faces"].shape[0], f["verts"].shape[0]
    c2ws, mask = _cu(f["c2ws_p"]), torch.zeros(3, Fn, dtype=torch.uint8, device="cuda")
    call = ctx.lib.utx_visible_faces_rays
    assert call(ctx.handle, bvh.handle, ptr(bvh.verts), ptr(bvh.faces), Fn - 1, ptr(c2ws), 3, 1, 0, ptr(mask), None, ctx.stream()) == -2
    assert call(ctx.handle, bvh.handle, None, ptr(bvh.faces), Fn, ptr(c2ws), 3, 1, 0, ptr(mask), None, ctx.stream()) == -2
    assert call(ctx.handle, bvh.handle, ptr(bvh.verts), ptr(bvh.faces), Fn, ptr(c2ws), 3, 1, 0, ptr(mask), None, ctx.stream()) == 0
    rast2d = torch.zeros(4 * 4 * 4 + 4, dtype=torch.float32, device="cuda")
    ndc, uv, alpha = torch.zeros(3, V, 2, device="cuda"), torch.zeros(3, 4, 4, 2, device="cuda"), torch.zeros(3, 4, 4, 1, device="cuda")
    m, rm, mo = torch.zeros(2, 4, 4, 3, device="cuda"), torch.zeros(3, 4, 4, 4, device="cuda"), torch.zeros(3, 4, 4, 3, device="cuda")
    up = ctx.lib.utx_uv_project
    faces = _faces(f)
    args = lambda r, Bm, F_=Fn, V_=V: (ctx.handle, r, ptr(faces), F_, ptr(mask), ptr(ndc), V_, 3, 4, 4, ptr(m), Bm, 4, 4, 3, ptr(rm), 0, 0, 0.0, None,
                                       ptr(uv), ptr(alpha), ptr(mo), ctx.stream())
    assert up(*args(C.c_void_p(rast2d.data_ptr() + 4), 1)) == -2          # a misaligned rast2d
    assert up(*args(ptr(rast2d), 2)) == -2                                 # Bm not in {1, B}
    assert up(*args(ptr(rast2d), 1, F_=0)) == -2 and up(*args(ptr(rast2d), 1, V_=0)) == -2
    assert up(*args(None, 1)) == -2
    assert up(*args(ptr(rast2d), 1)) == 0
    torch.cuda.synchronize()
