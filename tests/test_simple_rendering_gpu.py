"""Screen-space buffers on the GPU: utx_screen_gbuffer / ops.screen_gbuffer / NVDiffRendererInverse.simple_rendering against the reference's own
buffers (fixture G18), against the numpy restatement in the kernel's order, against the existing per-buffer kernels, and at the edges.
Bounds: the docstring of oracle/gbuffer_ref.py -- bit-exact for mask, alpha, the pure interpolations, v_attr, every background form
and map_attr in 'nearest' and 'nvdiffrast'; 5 u for the two normal buffers; 5 u * d / 7 u / 20 u for distance / ray_direction / cos_ray_normal;
MAP_BOUND = (14 M + 4 (W + H) R) u for 'bilinear' map_attr, whose reference is torch's CPU grid_sample (derivation there; the largest deviation
from the fixture is 12 u on the 16 x 24 map and 2 u on the 8 x 8 one, and the kernel is bit-identical to the restatement that shows it).
End to end the per-view vertex arrays are this build's own (utx_transform_points, utx_camera_normals in place of torch.matmul): the
camera-space buffers and z_depth then carry the matmul-order terms of oracle/gbuffer_ref.py (E2E_POS_ULPS, E2E_NRM_ULPS)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gbuffer_ref as GB
from oracle.pixel_ref import len3, sample

pytestmark = pytest.mark.gpu
F32, F64, U = np.float32, np.float64, GB.U
(H, W), B = GB.SCREEN, GB.VIEWS
ALL = ("mask", "alpha") + GB.GEOMETRY + ("v_attr", "uv", "map_attr")


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _direct(f, tag, want, **kw):
    """ops.screen_gbuffer on the fixture's rasters and the per-vertex arrays the reference handed to dr.interpolate"""
    from unitex_amd.texturetools import ops
    args = dict(v_nrm=_cu(f["v_nrm"]), v_uv=_cu(GB.v_uv(f)), clip_w=_cu(f["clip_w_" + tag]), v_pos_cam=_cu(f["v_pos_cam_" + tag]),
                v_nrm_cam=_cu(f["v_nrm_cam_" + tag]))
    for k in ("v_attr", "maps", "background"):
        if k in kw and kw[k] is not None and not isinstance(kw[k], float):
            kw[k] = tuple(_cu(m) for m in kw[k]) if k == "maps" else _cu(kw[k])
    if "mode" in kw:
        kw["filter"] = kw.pop("mode")
    args.update(kw)
    return _np(ops.screen_gbuffer(_cu(f["rast_" + tag]), _cu(f["faces"], torch.int32), _cu(f["verts"]), want=want, **args))


def _same(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    assert np.isfinite(got).all(), name
    assert got.tobytes() == want.tobytes(), "%s: max|diff| %.3g" % (name, np.abs(got.astype(F64) - want.astype(F64)).max())


def _renderer(f):
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    inv = NVDiffRendererInverse(device="cuda:0").update_from_arrays(f["verts"], f["faces"], f["uvs"])
    inv.pbr_mesh.set_vertex_normals(f["v_nrm"])
    return inv


def _cams(f, tag):
    return torch.from_numpy(f["c2ws_" + tag]), torch.from_numpy(f["intr_" + tag])


def _e2e_bound(f, tag, key, ref):
    """the bound of a buffer computed from this build's own per-view vertex arrays (matmul-order terms of oracle/gbuffer_ref.py)"""
    b = GB.bounds(key, ref["distance"])
    view = {"c2ws_" + tag: f["c2ws_" + tag], "verts": f["verts"]}
    smax = GB.pos_smax(view, tag)
    dpos = np.sqrt(3.0) * GB.E2E_POS_ULPS * U * smax
    if key == "z_depth":          # clip w: a row of the 4 x 4 mvp, <= 8 u * S per vertex and two interpolations of <= INTERP_ULPS each
        mvp_w = np.abs(f["clip_w_" + tag]).max()
        return GB.E2E_POS_ULPS * U * max(float(mvp_w), smax)
    if key in ("camera_position",):
        return dpos / np.sqrt(3.0)
    if key in ("distance", "ray_direction", "camera_normal", "cos_ray_normal"):
        dist = np.maximum(ref["distance"].astype(F64), 1e-30)
        drd = 2.0 * dpos / dist
        plen = len3(GB.interp_views(f["v_nrm_cam_" + tag].astype(F64), f["rast_" + tag], f["faces"]).astype(F64))
        dcn = 2.0 * np.sqrt(3.0) * GB.E2E_NRM_ULPS * U / np.maximum(plen, 1e-30)
        return b + {"distance": dpos, "ray_direction": drd, "camera_normal": dcn, "cos_ray_normal": drd + dcn}[key]
    return b


@pytest.mark.parametrize("tag", GB.SETS)
def test_g18_screen_gbuffer_on_fixture_rasters_and_arrays(tag):
    """one launch, every buffer: against the fixture within the bounds, and bit for bit against the restatement in the kernel's order"""
    f = GB.load_g18()
    maps = (f["map_0"], f["map_1"])
    got = _direct(f, tag, ALL, v_attr=f["v_attr"][:, :4], maps=maps)
    cov = f["rast_" + tag][..., 3] > 0
    assert got["mask"].dtype == np.uint8 and np.array_equal(got["mask"].astype(bool), cov)
    _same("alpha", got["alpha"], cov.astype(F32)[..., None])
    for k in GB.GEOMETRY + ("uv",):
        GB.check("direct %s %s" % (k, tag), got[k], f["%s_%s" % (k, tag)], GB.bounds(k, f["distance_" + tag]), cov)
    GB.check("direct v_attr " + tag, got["v_attr"], f["v_attr4_" + tag], 0.0, cov)
    GB.check("direct map_attr " + tag, got["map_attr"], np.concatenate([f["map_%d_bilinear_%s" % (i, tag)] for i in range(2)], -1),
             GB.map_bound("bilinear", maps), cov)
    want = GB.table(f["rast_" + tag], f["faces"], f["verts"], f["v_nrm"], f["v_pos_cam_" + tag], f["v_nrm_cam_" + tag], f["clip_w_" + tag], GB.v_uv(f),
                    f["v_attr"][:, :4], maps)
    for k in ALL:
        _same("restatement %s %s" % (k, tag), got[k], want[k].astype(np.uint8) if k == "mask" else want[k])


@pytest.mark.parametrize("tag", GB.SETS)
def test_g18_map_attr_modes_and_background_forms(tag):
    """each map alone and the tuple in the three filter modes; None, a float, a [C] vector and a dense image as background"""
    f = GB.load_g18()
    cov = f["rast_" + tag][..., 3] > 0
    for mode in GB.MODES:
        single = []
        for i in range(2):
            m = f["map_%d" % i]
            one = _direct(f, tag, ("map_attr",), maps=(m,), mode=mode)["map_attr"]
            GB.check("map_%d %s %s" % (i, mode, tag), one, f["map_%d_%s_%s" % (i, mode, tag)], GB.map_bound(mode, (m,)), cov)
            _same("restatement map_%d %s" % (i, mode), one, GB.table(f["rast_" + tag], f["faces"], v_uv=GB.v_uv(f), maps=(m,), mode=mode)["map_attr"])
            single.append(one)
        both = _direct(f, tag, ("map_attr",), maps=(f["map_0"], f["map_1"]), mode=mode)["map_attr"]
        _same("tuple " + mode, both, np.concatenate(single, -1))
    for key, kw, buf in GB.background_cases(f, tag):
        bound = GB.map_bound(kw.get("mode", "bilinear"), kw["maps"]) if buf == "map_attr" else 0.0
        kw = {k: v for k, v in kw.items() if k != "v_uv"}
        GB.check(key, _direct(f, tag, (buf,), **kw)[buf], f[key], bound, cov)


@pytest.mark.parametrize("tag", GB.SETS)
def test_g18_simple_rendering_end_to_end(tag):
    """the public method with its own cameras, rasters and per-view vertex arrays: the reference's keys, shapes and dtypes; the rasters equal the
    fixture's in (u, v, id), the precondition of every bound"""
    f = GB.load_g18()
    inv = _renderer(f)
    c2ws, intr = _cams(f, tag)
    persp = tag == "p"
    flags = {"render_" + k: True for k in GB.GEOMETRY + ("v_attr", "uv", "map_attr")}
    maps = (torch.from_numpy(f["map_0"])[None], torch.from_numpy(f["map_1"]))
    out = inv.simple_rendering(c2ws, intr, (H, W), perspective=persp, v_attr=f["v_attr"][:, :4], map_attr=maps, **flags)
    assert sorted(out) == sorted(ALL)
    assert out["mask"].dtype == torch.bool and tuple(out["mask"].shape) == (B, H, W, 1) and tuple(out["alpha"].shape) == (B, H, W, 1)
    rast = inv._view_raster(c2ws, intr, (H, W), persp)[4].cpu().numpy()
    assert np.array_equal(rast[..., [0, 1, 3]], f["rast_" + tag][..., [0, 1, 3]])
    cov = f["rast_" + tag][..., 3] > 0
    got = _np(out)
    assert np.array_equal(got["mask"][..., 0], cov) and np.array_equal(got["alpha"], cov.astype(F32)[..., None])
    ref = {k: f["%s_%s" % (k, tag)] for k in GB.GEOMETRY + ("uv",)}
    for k in GB.GEOMETRY + ("uv",):
        assert got[k].shape == (B, H, W, GB.CHANNELS[k]) and got[k].dtype == F32, k
        own = k in ("z_depth", "camera_normal", "camera_position", "distance", "ray_direction", "cos_ray_normal")
        GB.check("end to end %s %s" % (k, tag), got[k], ref[k], _e2e_bound(f, tag, k, ref) if own else GB.bounds(k, ref["distance"]), cov)
    GB.check("end to end v_attr", got["v_attr"], f["v_attr4_" + tag], 0.0, cov)
    GB.check("end to end map_attr", got["map_attr"], np.concatenate([f["map_%d_bilinear_%s" % (i, tag)] for i in range(2)], -1),
             GB.map_bound("bilinear", (f["map_0"], f["map_1"])), cov)
    # enable_antialis changes nothing; each flag alone is its slice of the all-flags call; an int render_size is a square screen
    again = inv.simple_rendering(c2ws, intr, (H, W), perspective=persp, v_attr=f["v_attr"][:, :4], map_attr=maps, enable_antialis=False, **flags)
    assert all(torch.equal(out[k], again[k]) for k in out)
    for k in GB.GEOMETRY + ("v_attr", "uv"):
        one = inv.simple_rendering(c2ws, intr, (H, W), perspective=persp, v_attr=f["v_attr"][:, :4], **{"render_" + k: True})
        assert sorted(one) == sorted(("mask", "alpha", k)) and torch.equal(one[k], out[k]), k
    for mode in GB.MODES:
        kw = dict(perspective=persp, render_uv=True, render_map_attr=True, grid_interpolate_mode=mode)
        single = [inv.simple_rendering(c2ws, intr, (H, W), map_attr=m, **kw)["map_attr"] for m in maps]
        both = inv.simple_rendering(c2ws, intr, (H, W), map_attr=maps, **kw)["map_attr"]
        assert torch.equal(both, torch.cat(single, -1)), mode
        if mode == "bilinear":
            assert torch.equal(both, out["map_attr"])
        else:
            GB.check("end to end map_0 " + mode, single[0].cpu().numpy(), f["map_0_%s_%s" % (mode, tag)], 0.0, cov)
    for key, kw, buf in GB.background_cases(f, tag)[2:]:
        r = inv.simple_rendering(c2ws, intr, (H, W), perspective=persp, v_attr=kw.get("v_attr"), map_attr=kw.get("maps"), render_v_attr=buf == "v_attr",
                                 render_uv=buf == "map_attr", render_map_attr=buf == "map_attr", grid_interpolate_mode=kw.get("mode", "bilinear"),
                                 background=kw["background"] if isinstance(kw["background"], float) else torch.from_numpy(kw["background"]))
        GB.check("end to end " + key, r[buf].cpu().numpy(), f[key], GB.map_bound(kw.get("mode", "bilinear"), kw["maps"]) if buf == "map_attr" else 0.0, cov)
    sq = inv.simple_rendering(c2ws, intr, 24, perspective=persp, render_uv=True)
    assert tuple(sq["uv"].shape) == (B, 24, 24, 2) and tuple(sq["mask"].shape) == (B, 24, 24, 1)


def test_one_launch_equals_the_composition():
    """every buffer bit for bit what callers could already compute: ops.transform_points / ops.camera_normals for the per-view vertex arrays,
    ops.interpolate per attribute, and torch's float32 elementwise operations (one rounding each) in the kernel's order"""
    from unitex_amd.texturetools import camera, ops
    f = GB.load_g18()
    inv = _renderer(f)
    m = inv.pbr_mesh
    c2ws, intr = _cams(f, "p")
    mvp, _, clip, _, rast = inv._view_raster(c2ws, intr, (H, W), True)
    a4 = _cu(f["v_attr"][:, :4])
    out = ops.screen_gbuffer(rast, m.faces, m.vertices, v_nrm=m.vertex_normals, v_uv=m.uvs_2d, v_attr=a4, mvp=mvp, c2ws=c2ws,
                             want=[k for k in ALL if k != "map_attr"])
    cov = rast[..., 3] > 0
    pcam = ops.transform_points(m.vertices, camera.c2w_to_w2c(c2ws).cuda().contiguous(), want_ndc=False)[0][..., :3].contiguous()
    ncam = ops.camera_normals(m.vertex_normals, c2ws.cuda().contiguous())
    interp = lambda attr, b: ops.interpolate(attr.contiguous(), rast[b], m.faces)
    sel = lambda x, fill: torch.where(cov[..., None], x, torch.full_like(x, fill))
    ln = lambda p: torch.sqrt((p[..., 0:1] * p[..., 0:1] + p[..., 1:2] * p[..., 1:2]) + p[..., 2:3] * p[..., 2:3])
    unit = lambda p: p / torch.clamp(ln(p), min=1e-12)
    stack = lambda fn: torch.stack([fn(b) for b in range(B)])
    assert torch.equal(out["mask"], cov.to(torch.uint8)) and torch.equal(out["alpha"], cov.float()[..., None])
    p = stack(lambda b: interp(pcam[b], b))
    cn, rd = unit(stack(lambda b: interp(ncam[b], b))), unit(p)
    want = {"z_depth": stack(lambda b: interp(clip[b, :, 3:], b)), "world_normal": sel(unit(stack(lambda b: interp(m.vertex_normals, b))), -1.0),
            "camera_normal": sel(cn, -1.0), "world_position": sel(stack(lambda b: interp(m.vertices, b)), -1.0), "camera_position": p,
            "distance": ln(p), "ray_direction": sel(rd, -1.0),
            "cos_ray_normal": sel((cn[..., 0:1] * rd[..., 0:1] + cn[..., 1:2] * rd[..., 1:2]) + cn[..., 2:3] * rd[..., 2:3], -1.0),
            "v_attr": stack(lambda b: interp(a4, b)), "uv": sel(stack(lambda b: interp(m.uvs_2d, b)), -1.0)}
    for k, w in want.items():
        assert torch.equal(out[k], w), "%s: max|diff| %.3g" % (k, (out[k] - w).abs().max().item())


def test_atlas_v_attr_and_unchanged_g17_calls():
    from unitex_amd.texturetools import ops
    f, g = GB.load_g18(), GB.load_g17()
    inv = _renderer(f)
    out = inv.simple_inverse_rendering(None, GB.ATLAS, render_v_attr=True, v_attr=f["v_attr"][:, :4], background=0.5)
    assert sorted(out) == ["alpha", "mask", "v_attr"]
    assert np.array_equal(inv._uv_raster(*GB.ATLAS).cpu().numpy()[..., [0, 1, 3]], f["atlas_rast"][..., [0, 1, 3]])
    GB.check("atlas v_attr", out["v_attr"].cpu().numpy(), f["atlas_v_attr4_half"], 0.0, f["atlas_rast"][None][..., 3] > 0)
    none = inv.simple_inverse_rendering(None, GB.ATLAS, render_v_attr=True, v_attr=f["v_attr"][:, :1])["v_attr"]
    assert tuple(none.shape) == (1,) + GB.ATLAS + (1,) and (none[~out["mask"][..., 0]] == 0).all()
    # the calls of G17 return what ops.uv_gbuffer returns, v_attr or not
    inv = _renderer(g)
    flags = {"render_" + k: True for k in GB.WORLD + GB.PER_VIEW}
    c2ws = torch.from_numpy(g["c2ws_o"])
    got = inv.simple_inverse_rendering(c2ws, GB.ATLAS, **flags)
    with_attr = inv.simple_inverse_rendering(c2ws, GB.ATLAS, render_v_attr=True, v_attr=torch.ones(len(g["verts"]), 2), **flags)
    m = inv.pbr_mesh
    want = ops.uv_gbuffer(inv._uv_raster(*GB.ATLAS), m.faces, m.vertices, m.vertex_normals, c2ws=c2ws, want=("mask", "alpha") + GB.WORLD + GB.PER_VIEW)
    assert sorted(got) == sorted(want) and sorted(with_attr) == sorted(list(want) + ["v_attr"])
    for k in want:
        w = want[k].bool()[None, ..., None] if k == "mask" else want[k][None] if k == "alpha" else want[k]
        assert torch.equal(got[k], w) and torch.equal(with_attr[k], w), k
    assert np.array_equal(got["world_position"].cpu().numpy(), g["world_position"])


def test_refusals():
    f = GB.load_g18()
    inv = _renderer(f)
    cam = _cams(f, "p") + ((H, W),)
    for flag in GB.UNBUILT:
        with pytest.raises(NotImplementedError, match=flag):
            inv.simple_rendering(*cam, **{flag: True})
        assert sorted(inv.simple_rendering(*cam, **{flag: False})) == ["alpha", "mask"]
    with pytest.raises(TypeError, match="render_albedo"):
        inv.simple_rendering(*cam, render_albedo=True)
    with pytest.raises(ValueError):
        inv.simple_rendering(*cam, render_uv=True, render_map_attr=True)
    with pytest.raises(ValueError):
        inv.simple_rendering(*cam, render_v_attr=True)
    with pytest.raises(ValueError):
        inv.simple_rendering(*cam, render_uv=True, render_map_attr=True, map_attr=(torch.zeros(2, 2, 1),) * 5)
    with pytest.raises(ValueError):
        inv.simple_rendering(*cam, render_v_attr=True, v_attr=torch.zeros(len(f["verts"]) + 1, 2))
    with pytest.raises(ValueError):
        inv.simple_inverse_rendering(None, GB.ATLAS, render_v_attr=True, v_attr=torch.zeros(len(f["verts"]) + 1, 2))


def test_edges():
    f = GB.load_g18()
    inv = _renderer(f)
    c2ws, intr = _cams(f, "p")
    flags = {"render_" + k: True for k in GB.GEOMETRY + ("v_attr", "uv", "map_attr")}
    kw = dict(v_attr=f["v_attr"], map_attr=torch.from_numpy(f["map_1"]), background=0.25, **flags)
    allb = inv.simple_rendering(c2ws, intr, (H, W), **kw)
    # B = 1: the first view of the batch
    one = inv.simple_rendering(c2ws[:1], intr, (H, W), **kw)
    assert all(tuple(one[k].shape[:3]) == (1, H, W) and torch.equal(one[k][0], allb[k][0]) for k in allb)
    # a camera moved 50 units along its own x axis: the mesh is far outside its frustum, every buffer is its background, nothing is NaN
    away = c2ws[:1].clone()
    away[0, :3, 3] = away[0, :3, 3] + 50.0 * away[0, :3, 0]
    out = _np(inv.simple_rendering(away, intr, (H, W), **kw))
    assert not out["mask"].any() and (out["alpha"] == 0).all()
    for k in GB.GEOMETRY + ("uv",):
        assert (out[k] == GB.FILL[k]).all(), k
    assert (out["v_attr"] == 0.25).all() and (out["map_attr"] == 0.25).all()
    out = _np(inv.simple_rendering(away, intr, (H, W), **dict(kw, background=None)))
    assert (out["v_attr"] == 0).all()
    _same("background sample", out["map_attr"], np.broadcast_to(sample(f["map_1"], np.full((1, 1, 1, 2), -1.0, F32), "bilinear"), out["map_attr"].shape).astype(F32))
    # a 1 x 1 map: zero padding blends it towards 0 (bilinear), wrap returns it everywhere, nearest returns it or the padding
    dot = np.array([[[0.5, -2.0]]], F32)
    for mode in GB.MODES:
        got = _direct(f, "p", ("map_attr",), maps=(dot,), mode=mode)["map_attr"]
        _same("1 x 1 " + mode, got, GB.table(f["rast_p"], f["faces"], v_uv=GB.v_uv(f), maps=(dot,), mode=mode)["map_attr"])
    assert (_direct(f, "p", ("map_attr",), maps=(dot,), mode="nvdiffrast")["map_attr"] == dot[0, 0]).all()
    # a screen whose size is no multiple of the block, in one view
    from unitex_amd.texturetools import ops
    r = inv._view_raster(c2ws[:1], intr, (33, 17), True)[4]
    got = _np(ops.screen_gbuffer(r, inv.pbr_mesh.faces, inv.pbr_mesh.vertices, v_uv=inv.pbr_mesh.uvs_2d, v_attr=_cu(f["v_attr"]), want=("mask", "uv", "v_attr")))
    want = GB.table(r.cpu().numpy(), f["faces"], v_uv=GB.v_uv(f), v_attr=f["v_attr"])
    assert got["mask"].any() and not got["mask"].all()
    _same("33 x 17 uv", got["uv"], want["uv"])
    _same("33 x 17 v_attr", got["v_attr"], want["v_attr"])
    # B = 0 and an empty screen: empty tensors, nothing launched
    z = ops.screen_gbuffer(r[:0], inv.pbr_mesh.faces, inv.pbr_mesh.vertices, v_uv=inv.pbr_mesh.uvs_2d, want=("mask", "uv"))
    assert tuple(z["uv"].shape) == (0, 33, 17, 2)


def _abi(ctx, f, want, outs, **kw):
    from unitex_amd._lib import ptr
    from unitex_amd.texturetools import ops
    a = dict(rast=_cu(f["rast_p"]), faces=_cu(f["faces"], torch.int32), v_pos=_cu(f["verts"]), v_nrm=_cu(f["v_nrm"]), v_uv=_cu(GB.v_uv(f)),
             v_attr=_cu(f["v_attr"]), Ca=7, clip_w=_cu(f["clip_w_p"]), v_pos_cam=_cu(f["v_pos_cam_p"]), v_nrm_cam=_cu(f["v_nrm_cam_p"]),
             V=len(f["verts"]), B=B, H=H, W=W, maps=[_cu(f["map_0"])], dims=[16, 24, 3], filter=0, bg_kind=0, bg_scalar=0.0, bg_v=None, bg_m=None, bits=None,
             maps_null=False)
    a.update(kw)
    ptrs = (C.c_void_p * len(ops.SCREEN_GBUFFERS))()
    for k, t in outs.items():
        ptrs[ops.SCREEN_GBUFFERS[k][0]] = t.data_ptr() if t is not None else None
    bits = sum(1 << ops.SCREEN_GBUFFERS[k][0] for k in want) if a["bits"] is None else a["bits"]
    n = len(a["maps"])
    mptr = (C.c_void_p * max(n, 1))(*[m.data_ptr() if m is not None else None for m in a["maps"]])
    mdim = (C.c_int * max(3 * n, 1))(*a["dims"])
    rc = ctx.lib.utx_screen_gbuffer(ctx.handle, ptr(a["rast"]), ptr(a["faces"]), ptr(a["v_pos"]), ptr(a["v_nrm"]), ptr(a["v_uv"]), ptr(a["v_attr"]), a["Ca"],
                                    ptr(a["clip_w"]), ptr(a["v_pos_cam"]), ptr(a["v_nrm_cam"]), a["V"], a["B"], a["H"], a["W"], n,
                                    None if a["maps_null"] else mptr, mdim, a["filter"], a["bg_kind"], a["bg_scalar"], ptr(a["bg_v"]), ptr(a["bg_m"]), bits,
                                    ptrs, ctx.stream())
    torch.cuda.synchronize()
    return rc


def test_error_codes_through_the_c_abi():
    """argument checks in front of the launch: a negative code and a message in utx_last_error, nothing reaches the device"""
    from unitex_amd.flux.ops import get_ctx
    f = GB.load_g18()
    ctx = get_ctx(0)
    npix = B * H * W
    bufs = {"z_depth": torch.empty(npix, device="cuda"), "camera_normal": torch.empty(npix * 3, device="cuda"),
            "v_attr": torch.empty(npix * 7, device="cuda"), "map_attr": torch.empty(npix * 3, device="cuda"), "uv": torch.empty(npix * 2, device="cuda")}
    want = tuple(bufs)
    call = lambda **kw: _abi(ctx, f, kw.pop("want", want), kw.pop("outs", bufs), **kw)
    assert call() == 0
    m0 = _cu(f["map_0"])
    bad = [dict(outs=dict(bufs, z_depth=None)),                                  # a requested buffer without a pointer
           dict(clip_w=None), dict(v_nrm_cam=None), dict(v_uv=None), dict(v_attr=None), dict(rast=None), dict(faces=None),
           dict(B=0),                                                            # per-view vertex arrays of no view
           dict(maps=[m0] * 5, dims=[16, 24, 3] * 5),                            # a fifth map
           dict(maps=[], dims=[]), dict(maps=[None]), dict(maps_null=True),
           dict(dims=[0, 24, 3]), dict(dims=[16, 0, 3]), dict(dims=[16, 24, 0]), dict(dims=[16, 24, -1]),      # a map with a zero side, a channel count <= 0
           dict(Ca=0), dict(Ca=-3), dict(H=-1), dict(W=-1), dict(B=-1), dict(V=0), dict(filter=3), dict(filter=-1), dict(bg_kind=4),
           dict(bg_kind=2), dict(bg_kind=3, bg_v=torch.zeros(npix * 7, device="cuda")),      # a vector / dense background without its pointer
           dict(bits=1 << 13)]                                                   # an unknown bit
    for kw in bad:
        assert call(**kw) == -2, kw
        assert b"utx_screen_gbuffer" in ctx.lib.utx_last_error(ctx.handle), kw
    assert call(rast=_cu(f["rast_p"]).view(-1)[1:]) == -2                         # read as float4: off a 16-byte boundary
    # nothing to do is no error, and writes nothing
    sent = {k: torch.full_like(t, -77.0) for k, t in bufs.items()}
    assert call(outs=sent, H=0) == 0 and call(outs=sent, bits=0) == 0
    assert call(outs=sent, want=("uv",), B=0) == 0
    assert all((t == -77.0).all() for t in sent.values())
