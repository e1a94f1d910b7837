"""Silhouette antialiasing on the GPU: utx_antialias_analyze / utx_antialias_apply / ops.antialias against the float32 numpy restatement
(tests/support/antialias_ref.py) byte for byte -- weights and outputs --, the refusals of the C ABI, and simple_rendering(antialias=True) against the
composition of its antialias=False buffers, torch.lerp and ops.antialias written out here, and against fixture G27 (the reference's own
simple_rendering(enable_antialis=True) with dr.antialias bound to the restatement).  The float32-against-float64 figures are the CPU test's
(tests/test_antialias_cpu.py): the kernel inherits them through bit-equality."""
import numpy as np
import pytest
import torch

from tests.support import antialias_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = ((1, 1), (1, 2), (2, 1), (3, 64), (5, 65), (17, 63), (64, 257))
BATCHES = ((1, False), (3, False), (3, True))      # (B, one pos per view?)
CHANNELS = (1, 3, 4, 7)


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _same(name, got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), "%s: %d elements differ, max|diff| %.3g" % (
        name, int((got != want).sum()), np.abs(got.astype(np.float64) - want.astype(np.float64)).max())


@pytest.mark.parametrize("batch", BATCHES, ids=["B1", "B3shared", "B3perview"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", R.CASES)
def test_bit_equal_to_the_float32_restatement(name, shape, batch):
    """every case on every screen in every batch form; all four channel counts on one set of weights"""
    from unitex_amd.texturetools import ops
    H, W = shape
    B, per_view = batch
    case = R.render_case(name, H, W, B=B, per_view=per_view, C=max(CHANNELS))
    rast, pos, tri, opp = _cu(case["rast"]), _cu(case["pos"]), _cu(case["tri"]), _cu(case["opp"])
    want_w, _ = R.weights(case["rast"], case["pos"], case["tri"], case["opp"])
    got_w = ops.antialias_weights(rast, pos, tri, opp)
    _same("weights", got_w, want_w)
    if name == "empty":
        assert not want_w.any()
    elif H >= 17:
        assert want_w.any(), "the case blends nothing on this screen"
    for C in CHANNELS:
        color = np.ascontiguousarray(case["color"][..., :C])
        want = R.apply(color, want_w)
        got = ops.antialias(_cu(color), rast, pos, tri, opp)
        _same("antialias C=%d" % C, got, want)
        assert torch.equal(ops.antialias_apply(_cu(color), got_w), got)
    if B == 1:      # the unbatched forms, and the topology computed from tri
        color = np.ascontiguousarray(case["color"][0, ..., :3])
        got = ops.antialias(_cu(color), rast[0], pos, tri)
        _same("unbatched, opp=None", got, R.apply(color[None], want_w)[0])


def test_weights_of_another_origin_stay_inside_the_buffer():
    """the stencil ignores a weight whose neighbour lies outside the view, as the restatement does"""
    from unitex_amd.texturetools import ops
    rng = np.random.default_rng(5)
    color = rng.uniform(-1, 1, (2, 3, 5, 2)).astype(F32)
    w = rng.uniform(0, 0.5, (2, 3, 5, 4)).astype(F32)
    _same("apply", ops.antialias_apply(_cu(color), _cu(w)), R.apply(color, w))


def test_error_codes_through_the_c_abi():
    from unitex_amd.texturetools import ops
    from unitex_amd._lib import ptr
    ctx = ops.get_ctx(0)
    case = R.render_case("triangle", 5, 65)
    rast, pos, tri, opp = _cu(case["rast"]), _cu(case["pos"]), _cu(case["tri"]), _cu(case["opp"])
    color = _cu(case["color"])
    w = torch.full((1, 5, 65, 4), 7.0, device="cuda")
    out = torch.full_like(color, 7.0)
    F, V = tri.shape[0], pos.shape[0]
    lib, s = ctx.lib, ctx.stream()
    good = (ptr(rast), ptr(pos), 0, ptr(tri), ptr(opp), F, V, 1, 5, 65, ptr(w), s)
    for i in (0, 1, 3, 4, 10):      # a null pointer in each pointer slot
        assert lib.utx_antialias_analyze(ctx.handle, *[None if k == i else a for k, a in enumerate(good)]) == -2, i
    for i in (5, 6, 7, 8, 9):      # a non-positive size
        assert lib.utx_antialias_analyze(ctx.handle, *[0 if k == i else a for k, a in enumerate(good)]) == -2, i
    assert lib.utx_antialias_analyze(ctx.handle, *[4 * V + 4 if k == 2 else a for k, a in enumerate(good)]) == -2
    big = torch.zeros(1 * 5 * 65 * 4 + 4, device="cuda")
    assert lib.utx_antialias_analyze(ctx.handle, *[big.data_ptr() + 4 if k == 0 else a for k, a in enumerate(good)]) == -2      # rast off 16 bytes
    assert lib.utx_antialias_analyze(ctx.handle, *[big.data_ptr() + 8 if k == 10 else a for k, a in enumerate(good)]) == -2      # weights off 16 bytes
    torch.cuda.synchronize()
    assert (w == 7.0).all()
    assert lib.utx_antialias_analyze(ctx.handle, *good) == 0
    C = color.shape[-1]
    fine = (ptr(color), ptr(w), 1, 5, 65, C, ptr(out), s)
    for i in (0, 1, 6):
        assert lib.utx_antialias_apply(ctx.handle, *[None if k == i else a for k, a in enumerate(fine)]) == -2, i
    for i in (2, 3, 4, 5):
        assert lib.utx_antialias_apply(ctx.handle, *[0 if k == i else a for k, a in enumerate(fine)]) == -2, i
    assert lib.utx_antialias_apply(ctx.handle, *[ptr(color) if k == 6 else a for k, a in enumerate(fine)]) == -2      # out == color
    assert lib.utx_antialias_apply(ctx.handle, *[big.data_ptr() + 4 if k == 1 else a for k, a in enumerate(fine)]) == -2
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert lib.utx_antialias_apply(ctx.handle, *fine) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ops.antialias(color, rast, pos, tri, opp))


# ---- wiring
GEOMETRY = ("z_depth", "world_normal", "camera_normal", "world_position", "camera_position", "distance", "ray_direction", "cos_ray_normal")
FILL = dict(z_depth=0.0, world_normal=-1.0, camera_normal=-1.0, world_position=-1.0, camera_position=0.0, distance=0.0, ray_direction=-1.0,
            cos_ray_normal=-1.0, uv=-1.0)
SCREEN = (40, 48)


def _scene():
    """the 80-face sphere with one fin (a border edge in front of the surface), spherical UVs, a 4-channel vertex attribute and a 16 x 24 x 3 map"""
    verts, faces = R._icosphere()
    verts = 0.8 * verts
    fin = np.array([[0.0, 0.0, 0.8], [0.5, 0.9, 1.0], [-0.6, 0.7, 1.0]])
    faces = np.concatenate([faces, [[len(verts), len(verts) + 1, len(verts) + 2]]]).astype(np.int32)
    verts = np.concatenate([verts, fin]).astype(F32)
    nrm = (verts / np.linalg.norm(verts, axis=1, keepdims=True)).astype(F32)
    uvs = np.stack([np.arctan2(nrm[:, 0], nrm[:, 2]) / (2 * np.pi) + 0.5, np.arccos(np.clip(nrm[:, 1], -1, 1)) / np.pi], 1).astype(F32)
    rng = np.random.default_rng(27)
    return verts, faces, uvs, nrm, rng.uniform(-1, 1, (len(verts), 4)).astype(F32), rng.uniform(0, 1, (16, 24, 3)).astype(F32)


def _cameras(perspective):
    from oracle import geom_ref
    c2ws = geom_ref.box_views_c2ws(2.8)[[0, 1]]
    intr = geom_ref.intrinsics(49.1, 49.1, fov=True, degree=True) if perspective else geom_ref.intrinsics(0.85, 0.85, fov=False)
    return torch.from_numpy(c2ws), torch.from_numpy(np.stack([intr, intr]))


@pytest.mark.parametrize("background", [None, 0.25, "vector"], ids=["none", "number", "vector"])
@pytest.mark.parametrize("perspective", [True, False], ids=["perspective", "orthographic"])
def test_simple_rendering_antialias_is_the_written_out_composition(perspective, background):
    from unitex_amd.texturetools import ops
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    verts, faces, uvs, nrm, v_attr, tex = _scene()
    inv = NVDiffRendererInverse(device="cuda:0").update_from_arrays(verts, faces, uvs)
    inv.pbr_mesh.set_vertex_normals(nrm)
    c2ws, intr = _cameras(perspective)
    flags = {"render_" + k: True for k in GEOMETRY + ("v_attr", "uv", "map_attr")}
    # v_attr has 4 channels and map_attr 3: a [C] background serves one of them at a time
    calls = [dict(flags)] if background != "vector" else [dict(flags, render_v_attr=False), dict(flags, render_map_attr=False)]
    for fl in calls:
        bg = background
        if background == "vector":
            bg = torch.tensor([0.1, 0.6, 0.3, 0.9][:3 if fl["render_map_attr"] else 4])
        kw = dict(perspective=perspective, v_attr=v_attr, map_attr=torch.from_numpy(tex), **fl)
        off = inv.simple_rendering(c2ws, intr, SCREEN, background=None, **kw)
        default = inv.simple_rendering(c2ws, intr, SCREEN, background=None, antialias=False, enable_antialis=True, **kw)
        assert sorted(off) == sorted(default) and all(off[k].cpu().numpy().tobytes() == default[k].cpu().numpy().tobytes() for k in off)
        on = inv.simple_rendering(c2ws, intr, SCREEN, background=bg, antialias=True, **kw)
        assert sorted(on) == sorted(off)
        # the composition, written out: one set of weights; alpha; then per buffer the reference's pre-blend and the stencil
        mvp, _, clip, _, rast = inv._view_raster(c2ws, intr, SCREEN, perspective)
        opp = _cu(R.edge_opposites(faces))
        aa = lambda x: ops.antialias(x.contiguous(), rast, clip, inv.pbr_mesh.faces, opp)
        mask = off["mask"]
        assert torch.equal(on["mask"], mask) and mask.any() and not mask.all()
        alpha = aa(mask.float())
        assert torch.equal(on["alpha"], alpha)
        edge = (alpha > 0) & (alpha < 1)
        assert (edge & mask).any() and (edge & ~mask).any()      # covered and uncovered edge pixels hold a coverage estimate
        raw = {k: torch.where(mask, off[k], torch.zeros_like(off[k])) for k in GEOMETRY + ("uv",)}
        want = {}
        for k in GEOMETRY + ("uv",):
            x = raw[k]
            if k == "distance":
                x = torch.norm(want["camera_position"], p=2, dim=-1, keepdim=True)
            if k == "ray_direction":
                x = torch.nn.functional.normalize(want["camera_position"], dim=-1)
            want[k] = aa(torch.lerp(torch.full_like(x, FILL[k]), x, alpha))
        for k in ("v_attr", "map_attr"):
            if not fl["render_" + k]:
                continue
            x = off[k]
            if bg is not None:
                full = torch.full_like(x, bg) if isinstance(bg, float) else bg.cuda().expand_as(x)
                x = torch.lerp(full, x, alpha)
            want[k] = aa(x)
        for k in want:
            assert on[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
            assert not torch.equal(on[k], off[k]), k
        # the alpha of the renderer is the restatement's on the renderer's own raster, byte for byte
        ref = R.antialias_f32(mask.float().cpu().numpy(), rast.cpu().numpy(), clip.cpu().numpy(), faces)
        assert on["alpha"].cpu().numpy().tobytes() == ref.tobytes()


def test_wrappers_pass_the_keyword_through():
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    verts, faces, uvs, nrm, v_attr, tex = _scene()
    inv = NVDiffRendererInverse(device="cuda:0").update_from_arrays(verts, faces, uvs)
    inv.pbr_mesh.set_vertex_normals(nrm)
    c2ws, intr = _cameras(True)
    g = inv.geometry_rendering(c2ws, intr, SCREEN, antialias=True)
    s = inv.simple_rendering(c2ws, intr, SCREEN, antialias=True, **{"render_" + k: True for k in GEOMETRY + ("uv",)})
    assert sorted(g) == sorted(s) and all(torch.equal(g[k], s[k]) for k in g)
    v = inv.vertex_rendering(v_attr, c2ws, intr, SCREEN, antialias=True, background=0.5)
    assert torch.equal(v["rgb"], inv.simple_rendering(c2ws, intr, SCREEN, v_attr=v_attr, render_v_attr=True, background=0.5, antialias=True)["v_attr"])
    u = inv.uv_rendering(torch.from_numpy(tex), c2ws, intr, SCREEN, antialias=True)
    assert torch.equal(u["rgb"], inv.simple_rendering(c2ws, intr, SCREEN, map_attr=torch.from_numpy(tex), render_uv=True, render_map_attr=True,
                                                      antialias=True)["map_attr"])
    assert not torch.equal(u["alpha"], inv.uv_rendering(torch.from_numpy(tex), c2ws, intr, SCREEN)["alpha"])
    for bad in (inv.global_inverse_rendering,):
        with pytest.raises(TypeError):
            bad(torch.zeros(2, 40, 48, 3), c2ws, intr, SCREEN, 64, antialias=True)


# ---- fixture G27: the reference's own simple_rendering(enable_antialis=True) with dr.antialias bound to the float32 restatement
U = 2.0 ** -24


def _spread(b):
    """the stencil's first-order propagation of a per-pixel input bound b [B,H,W,1]: out = c + sum_n w_n (c_n - c) with w_n <= 0.5 moves by at most
    (1 + 4 * 0.5) |dc| + 0.5 * sum_n |dc_n| <= 5 * the largest bound among the pixel and its four neighbours"""
    m = b.copy()
    m[:, :, 1:] = np.maximum(m[:, :, 1:], b[:, :, :-1]); m[:, :, :-1] = np.maximum(m[:, :, :-1], b[:, :, 1:])
    m[:, 1:] = np.maximum(m[:, 1:], b[:, :-1]); m[:, :-1] = np.maximum(m[:, :-1], b[:, 1:])
    return 5.0 * m


def _held(name, got, ref, bound):
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype and np.isfinite(got).all(), (name, got.shape, ref.shape)
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    if np.ndim(bound) == 0 and bound == 0.0:
        print("%s: max|diff| %.3g (bit-exact required)" % (name, d.max()))
        assert got.tobytes() == ref.tobytes(), name
        return
    bb = np.broadcast_to(np.asarray(bound, np.float64), d.shape)
    share = float((d / bb).max())
    print("%s: max|diff| %.3g = %.3g u, at most %.3f of the bound" % (name, d.max(), d.max() / U, share))
    assert share <= 1.0, "%s: max|diff| %.3g is %.3f of its bound" % (name, d.max(), share)


@pytest.mark.parametrize("tag", ["p", "o"])
def test_simple_rendering_antialias_equals_fixture_g27(tag):
    """simple_rendering(antialias=True), all eleven flags, against the reference's own buffers.  The renderer gets the fixture's rasters and clip-space
    vertices at its _view_raster seam (as the G18 tests feed the fixture's rasters to ops.screen_gbuffer), so alpha and the weights are the fixture's bit
    for bit; the camera-space per-vertex arrays are this build's own (utx_transform_points, utx_camera_normals).  Bounds, none taken from GPU output, in
    u = 2^-24: a buffer's raw value x carries dx (0 for the pure interpolations; oracle/gbuffer_ref.py's 5 u for normals, MAP_BOUND for 'bilinear',
    24 u SMAX for a camera-space coordinate, the normal and cosine terms of its docstring); torch.lerp is a + w (b - a) or b - (b - a)(1 - w), three
    roundings on either side, fused or not: L = 6 u (|fill| + max|x|); the stencil is one float32 sequence on both sides, so it carries its inputs'
    bound as _spread says plus 8 u max|x| for its own eight operations on perturbed values.  distance and ray_direction are taken from the antialiased
    camera position p' (renderer_base.py:245-256): |p'| moves by <= sqrt(3) dp' (+ 4 u |p'|), p' / |p'| by <= 2 sqrt(3) dp' / |p'| (+ 8 u), and the
    blend with alpha scales the latter by alpha."""
    from oracle import gbuffer_ref as GB
    from oracle.pixel_ref import len3
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    f = R.load_g27()
    H, W = R.G27_SCREEN
    inv = NVDiffRendererInverse(device="cuda:0").update_from_arrays(f["verts"], f["faces"], f["uvs"])
    inv.pbr_mesh.set_vertex_normals(f["v_nrm"])
    c2ws, intr = torch.from_numpy(f["c2ws_" + tag]), torch.from_numpy(f["intr_" + tag])
    persp = tag == "p"
    # precondition: this build's own rasters show the fixture's triangles with the fixture's barycentrics
    own = inv._view_raster(c2ws, intr, (H, W), persp)
    assert np.array_equal(own[4].cpu().numpy()[..., [0, 1, 3]], f["rast_" + tag][..., [0, 1, 3]])
    inv._view_raster = lambda *a, **k: (None, c2ws.float(), _cu(f["clip_" + tag]), None, _cu(f["rast_" + tag]))
    flags = {"render_" + k: True for k in GEOMETRY + ("v_attr", "uv", "map_attr")}
    kw = dict(perspective=persp, v_attr=f["v_attr"], map_attr=torch.from_numpy(f["map_0"]), antialias=True)
    out = inv.simple_rendering(c2ws, intr, (H, W), **kw, **flags)
    cov = f["rast_" + tag][..., 3:4] > 0
    assert torch.equal(out["mask"].cpu(), torch.from_numpy(cov))
    _held("alpha", out["alpha"], f["alpha_" + tag], 0.0)
    alpha = f["alpha_" + tag].astype(np.float64)
    assert ((alpha > 0) & (alpha < 1) & cov).any()
    smax = GB.pos_smax({"c2ws_" + tag: f["c2ws_" + tag], "verts": f["verts"]}, tag)
    dposc = GB.E2E_POS_ULPS * U * smax
    rast, faces = f["rast_" + tag], f["faces"]
    dist_raw = np.maximum(len3(GB.interp_views(f["v_pos_cam_" + tag].astype(np.float64), rast, faces, np.float64)), 1e-30)
    plen = np.maximum(len3(GB.interp_views(f["v_nrm_cam_" + tag].astype(np.float64), rast, faces, np.float64)), 1e-30)
    drd = np.where(cov, 2.0 * np.sqrt(3.0) * dposc / dist_raw, 0.0)
    dcn = np.where(cov, 2.0 * np.sqrt(3.0) * GB.E2E_NRM_ULPS * U / plen, 0.0)
    mb = float(np.max(GB.map_bound("bilinear", (f["map_0"],))))
    raw = {"z_depth": 0.0, "world_position": 0.0, "uv": 0.0, "v_attr": 0.0, "map_attr": mb, "world_normal": GB.NORMAL_ULPS * U * cov,
           "camera_position": dposc * cov, "camera_normal": GB.NORMAL_ULPS * U * cov + dcn, "cos_ray_normal": 2 * GB.COS_ULPS * U * cov + drd + dcn}
    full = lambda b: np.broadcast_to(np.asarray(b, np.float64), alpha.shape).copy()

    def after(k, dx, ref, fill):
        M = max(float(np.abs(ref).max()), abs(fill), smax if "position" in k or k == "distance" else 0.0)
        return _spread(full(dx) + 6.0 * U * (abs(fill) + M)) + 8.0 * U * M

    bound = {}
    for k in ("z_depth", "world_normal", "camera_normal", "world_position", "camera_position", "cos_ray_normal", "uv"):
        bound[k] = after(k, raw[k], f["%s_%s" % (k, tag)], FILL[k])
    cp = f["camera_position_" + tag].astype(np.float64)
    norm = np.sqrt((cp * cp).sum(-1, keepdims=True))
    bound["distance"] = after("distance", np.sqrt(3.0) * bound["camera_position"] + 4.0 * U * norm, f["distance_" + tag], 0.0)
    turn = np.where(norm > 0, alpha * 2.0 * np.sqrt(3.0) * bound["camera_position"] / np.maximum(norm, 1e-30), 0.0) + 8.0 * U
    bound["ray_direction"] = after("ray_direction", turn, f["ray_direction_" + tag], -1.0)
    for k in GEOMETRY + ("uv",):
        _held("%s %s" % (k, tag), out[k], f["%s_%s" % (k, tag)], bound[k])
    # v_attr / map_attr: no pre-blend without a background (the stencil alone), lerp with the float and the [C] backgrounds
    _held("v_attr " + tag, out["v_attr"], f["v_attr_" + tag], _spread(full(0.0)) + 8.0 * U)
    _held("map_attr " + tag, out["map_attr"], f["map_attr_" + tag], _spread(full(mb)) + 8.0 * U)
    r = inv.simple_rendering(c2ws, intr, (H, W), render_v_attr=True, render_uv=True, render_map_attr=True, background=R.G27_BG_FLOAT, **kw)
    _held("v_attr float " + tag, r["v_attr"], f["v_attr_float_" + tag], after("v_attr", 0.0, f["v_attr_float_" + tag], 1.0))
    _held("map_attr float " + tag, r["map_attr"], f["map_attr_float_" + tag], after("map_attr", mb, f["map_attr_float_" + tag], 1.0))
    r = inv.simple_rendering(c2ws, intr, (H, W), render_v_attr=True, background=torch.from_numpy(f["bg_vec_4"]), **kw)
    _held("v_attr vector " + tag, r["v_attr"], f["v_attr_vec_" + tag], after("v_attr", 0.0, f["v_attr_vec_" + tag], 1.0))
    r = inv.simple_rendering(c2ws, intr, (H, W), render_uv=True, render_map_attr=True, background=torch.from_numpy(f["bg_vec_3"]), **kw)
    _held("map_attr vector " + tag, r["map_attr"], f["map_attr_vec_" + tag], after("map_attr", mb, f["map_attr_vec_" + tag], 1.0))
    # distance and ray_direction alone: from the raw camera position (no render_camera_position), the counted bounds of the raw buffers
    r = inv.simple_rendering(c2ws, intr, (H, W), render_distance=True, render_ray_direction=True, **kw)
    assert sorted(r) == ["alpha", "distance", "mask", "ray_direction"]
    d_raw = np.where(cov, 2 * GB.DIST_ULPS * U * dist_raw + np.sqrt(3.0) * dposc, 0.0)
    _held("distance alone " + tag, r["distance"], f["distance_alone_" + tag], after("distance", d_raw, f["distance_alone_" + tag], 0.0))
    _held("ray_direction alone " + tag, r["ray_direction"], f["ray_direction_alone_" + tag],
          after("ray_direction", 2 * GB.UNIT_ULPS * U * cov + drd, f["ray_direction_alone_" + tag], -1.0))
    assert not torch.equal(r["distance"], out["distance"])
