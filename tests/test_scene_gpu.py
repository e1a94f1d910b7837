"""Environment renderer on the GPU (csrc/scene.hip) against the fp64 restatement of tests/support/scene_ref.py and the reference's own arrays (fixture G23).
Every bound is counted there from the kernels' operation sequences (its module docstring states each derivation); no GPU number enters a bound.
  rays_d, uv, bake uv   inside the counted bound around the restatement evaluated from the cameras (uv: with the conditioning of acos and of atan2)
  lookups               the restatement evaluated AT THE KERNEL'S OWN rays_d / uv: only the coordinate and blend roundings remain
  rays_o, masks, unseen texels, layouts: bit-exact."""
import numpy as np
import pytest
import torch

from oracle import pbr_ref as PC
from tests.support import scene_ref as S

pytestmark = pytest.mark.gpu
F32 = np.float32


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda().contiguous()


def _np(t):
    return t.cpu().numpy()


def _look(forward, up, eye=(0.0, 0.0, 0.0)):
    """c2w of a camera at `eye` looking along `forward` (the camera looks down its -z)"""
    z = -np.asarray(forward, np.float64)
    x = np.cross(up, z)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
    return m.astype(F32)


AXES = [((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (0, 0, 1)), ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0))]


def _orbit(n, radius=0.3, height=0.1):
    from unitex_amd.texturetools import camera
    return camera.generate_orbit_views_c2ws(n, radius=radius, height=height, theta_0=10.0, degree=True).to(torch.float32).numpy()


def _intr(fov=60.0):
    from unitex_amd.texturetools import camera
    return camera.generate_intrinsics(fov, fov, fov=True, degree=True).to(torch.float32).numpy()


def _check_render(c2ws, intr, H, W, cube, lat):
    """all four outputs of one launch against the restatement; returns the outputs"""
    from unitex_amd.texturetools import ops
    got = {k: _np(v) for k, v in ops.scene_render(_cu(c2ws), _cu(intr), H, W, cubemap=_cu(cube), latlong=_cu(lat),
                                                  want=("rays_d", "cubemap_attr", "uv", "latlong_map_attr")).items()}
    _, rd, bound = S.rays(c2ws, intr, H, W)
    e = np.abs(got["rays_d"] - rd).max(-1)
    print("rays_d: worst error / bound %.3f" % (e / bound).max())
    assert (e <= bound).all()
    uv, ub = S.dir_uv(rd), S.uv_bound(rd, bound[..., None][..., 0])
    eu, ev = S.circle_diff(got["uv"][..., 0], uv[..., 0]), np.abs(got["uv"][..., 1] - uv[..., 1])
    print("uv: worst error / bound %.3f, %.3f" % ((eu / ub[..., 0]).max(), (ev / ub[..., 1]).max()))
    assert (eu <= ub[..., 0]).all() and (ev <= ub[..., 1]).all()
    assert (got["uv"] >= 0).all() and (got["uv"] <= 1).all()
    ec = np.abs(got["cubemap_attr"] - PC.cube_lookup(cube, got["rays_d"])).max()
    el = np.abs(got["latlong_map_attr"] - S.wrap_linear(lat, got["uv"])).max()
    print("lookups at the kernel's own coordinates: cube %.3g (bound %.3g), lat-long %.3g (bound %.3g)" % (ec, S.cube_bound(cube), el, S.wrap_bound(lat)))
    assert ec <= S.cube_bound(cube) and el <= S.wrap_bound(lat)
    return got


# ---------------------------------------------------------------------------------------------------------------- perspective_rendering
@pytest.mark.parametrize("B,H,W,N,Hi,Wi,Cc", [(1, 1, 1, 2, 1, 2, 1), (3, 5, 7, 4, 6, 8, 3), (3, 8, 12, 4, 6, 12, 4), (1, 17, 33, 2, 6, 8, 3)])
def test_render_against_the_restatement(B, H, W, N, Hi, Wi, Cc):
    rng = np.random.default_rng(100 * B + H)
    cube, lat = rng.uniform(0, 1, (6, N, N, Cc)).astype(F32), rng.uniform(0, 1, (Hi, Wi, Cc)).astype(F32)
    c2ws = _orbit(B)
    intr = _intr()
    if B > 1:      # one matrix per camera, each different
        intr = np.stack([_intr(50.0 + 10.0 * b) for b in range(B)])
        intr[:, 0, 2] += 0.03
    _check_render(c2ws, intr, H, W, cube, lat)


@pytest.mark.parametrize("fx,size", [(0.5, 3), (0.375, 4)])
def test_seams_wrap_column_and_poles(fx, size):
    """Six cameras at the origin looking along +-x, +-y, +-z into an N = 2 cubemap.  fx = 0.5 (90 degrees), 3 x 3: the outer pixels sit at face coordinates
    +-2/3, past the last texel centre (+-1/2), so their taps leave the face along one axis (edges) and, in the view's corners, along both (the corner mean).
    fx = 0.375, 4 x 4: the outer pixels' rays pass exactly through the cube's edges and corners (face coordinate 0.75 / 0.75 = 1).  With an odd size the middle
    column of the +z camera has dx = 0, dz > 0 (phi = +-pi, the panorama's wrap column) and the middle pixels of the +-y cameras are the poles (0, +-1, 0)."""
    rng = np.random.default_rng(5)
    cube, lat = rng.uniform(0, 1, (6, 2, 2, 3)).astype(F32), rng.uniform(0, 1, (6, 8, 3)).astype(F32)
    c2ws = np.stack([_look(f, u) for f, u in AXES])
    intr = np.array([[fx, 0, 0.5], [0, fx, 0.5], [0, 0, 1]], F32)
    got = _check_render(c2ws, intr, size, size, cube, lat)
    d = got["rays_d"]
    if size % 2:
        mid = size // 2
        assert np.array_equal(d[2, mid, mid], [0, 1, 0]) and np.array_equal(d[3, mid, mid], [0, -1, 0]), "the poles"
        assert got["uv"][2, mid, mid, 1] == 0.0 and got["uv"][3, mid, mid, 1] == 1.0
        col = d[4, :, mid]
        assert (col[:, 0] == 0).all() and (col[:, 2] > 0).all(), "the wrap column"
        assert np.isin(got["uv"][4, :, mid, 0], [0.0, 1.0]).all()
        # both ends of the wrap column read the same texels
        assert np.abs(S.wrap_linear(lat, np.stack([np.zeros(size), got["uv"][4, :, mid, 1]], -1)) - got["latlong_map_attr"][4, :, mid]).max() <= S.wrap_bound(lat)
    else:
        a = np.abs(d)
        assert (np.sort(a, -1)[..., 1] == np.sort(a, -1)[..., 2]).sum() >= 6 * 12, "rays through the cube's edges"
        assert (a.max(-1) == a.min(-1)).sum() == 6 * 4, "rays through the cube's corners"


# ---------------------------------------------------------------------------------------------------------------- cubemap_to_latlong
@pytest.mark.parametrize("N,Ht,Wt,Cc", [(2, 1, 2, 1), (4, 6, 8, 3), (4, 6, 12, 4), (2, 17, 33, 3)])
def test_cubemap_to_latlong(N, Ht, Wt, Cc):
    from unitex_amd.texturetools import renderer_scene as RS
    cube = np.random.default_rng(N + Wt).uniform(0, 1, (6, N, N, Cc)).astype(F32)
    got = _np(RS.cubemap_to_latlong(_cu(cube), (Ht, Wt)))
    err = np.abs(got - S.cubemap_to_latlong(cube, Ht, Wt)).max()
    print("cubemap_to_latlong: %.3g (bound %.3g)" % (err, S.cubemap_to_latlong_bound(cube)))
    assert got.shape == (Ht, Wt, Cc) and err <= S.cubemap_to_latlong_bound(cube)
    # 0.75, 0.5, 0.25, 1: a + f (a - a) is exact and so is the corner mean ((c + c) + c) / 3 of a constant with two mantissa bits
    const = np.broadcast_to(np.array([0.75, 0.5, 0.25, 1.0], F32)[:Cc], (6, N, N, Cc)).copy()
    assert np.array_equal(_np(RS.cubemap_to_latlong(_cu(const), (Ht, Wt))), np.broadcast_to(const[0, 0, 0], (Ht, Wt, Cc)))


# ---------------------------------------------------------------------------------------------------------------- the bake
def _bake_case(M, H, W, Ht, Wt, Cc, seed):
    rng = np.random.default_rng(seed)
    from unitex_amd.texturetools import camera
    c2ws = torch.from_numpy(_orbit(5)[:M].copy())
    w2cs = torch.linalg.inv(c2ws).numpy()
    projs = camera.intr_to_proj(torch.from_numpy(_intr()), perspective=True).expand(M, 4, 4).contiguous().numpy()
    return w2cs, projs, rng.uniform(-0.2, 1.5, (M, H, W, Cc)).astype(F32)


@pytest.mark.parametrize("M,H,W,Ht,Wt,Cc", [(1, 1, 1, 1, 2, 1), (5, 5, 7, 6, 8, 3), (5, 8, 12, 6, 12, 4), (1, 5, 7, 17, 33, 3)])
def test_bake_against_the_restatement(M, H, W, Ht, Wt, Cc):
    from unitex_amd.texturetools import ops
    w2cs, projs, img = _bake_case(M, H, W, Ht, Wt, Cc, 7 * M + Wt)
    uv, depth, alpha, bound, dbound = S.bake_project(w2cs, projs, Ht, Wt)
    assert S.bake_margin_ok(uv, depth, bound, dbound), "the test's own cameras decide every mask with room to spare"
    g_uv, g_alpha, g_attr = (_np(t) for t in ops.scene_bake_latlong(_cu(w2cs), _cu(projs), Ht, Wt, _cu(img)))
    assert np.array_equal(g_alpha, alpha[..., None].astype(F32)), "uv_alpha: exact"
    behind = (depth < 0) & (np.abs(uv) <= 1).all(-1)
    if Ht * Wt > 2:
        assert behind.any() and (g_alpha[behind] == 0).all(), "a texel straight behind a camera projects inside the view and is refused by its depth"
    e = np.abs(g_uv - uv)
    print("bake uv: worst error / bound %.3f" % (e / bound).max())
    assert (e <= bound).all()
    want, cnt = S.bake(img, g_uv, g_alpha)
    unseen = cnt == 0
    assert np.array_equal(alpha.sum(0) == 0, unseen) and (g_attr[unseen] == 0).all(), "unseen texels: the same set, exact zeros"
    err = np.abs(g_attr - want).max(-1)
    print("baked panorama at the kernel's own uv: %.3g (bound %.3g); %d of %d texels seen" % (err.max(), S.bake_bound(img, cnt).max(), (~unseen).sum(), unseen.size))
    assert (err <= S.bake_bound(img, cnt)).all() and (g_attr >= 0).all() and (g_attr <= 1).all()
    # uv and uv_alpha alone (no images) are the same bits
    o_uv, o_alpha, o_attr = ops.scene_bake_latlong(_cu(w2cs), _cu(projs), Ht, Wt)
    assert o_attr is None and np.array_equal(_np(o_uv), g_uv, equal_nan=True) and np.array_equal(_np(o_alpha), g_alpha)


def test_bake_of_a_constant_image():
    """Where every view that sees a texel samples it inside the hull of its pixel centres (|u| <= 1 - 1 / W, |v| <= 1 - 1 / H: no tap is zero padding) the mean
    of M views of the constant c is c, to the bake's bound (the four weights do not sum to exactly 1 in fp32).  Nearer to a view's border the zero padding
    darkens the sample, in the reference too."""
    from unitex_amd.texturetools import ops
    M, H, W, Ht, Wt = 5, 8, 12, 6, 12
    w2cs, projs, _ = _bake_case(M, H, W, Ht, Wt, 3, 1)
    img = np.full((M, H, W, 3), 0.375, F32)
    uv, alpha, attr = (_np(t) for t in ops.scene_bake_latlong(_cu(w2cs), _cu(projs), Ht, Wt, _cu(img)))
    a = alpha[..., 0] > 0
    hull = (np.abs(uv[..., 0]) <= 1 - 1 / W) & (np.abs(uv[..., 1]) <= 1 - 1 / H)
    full = a.any(0) & (~a | hull).all(0)
    assert full.sum() >= 8
    assert np.abs(attr[full] - 0.375).max() <= S.bake_bound(img, a.sum(0)).max()
    assert (attr[~a.any(0)] == 0).all() and (attr <= 0.375 + S.bake_bound(img, a.sum(0)).max()).all()


# ---------------------------------------------------------------------------------------------------------------- the class
def test_class_flags_ops_and_constants():
    from unitex_amd.texturetools import ops
    from unitex_amd.texturetools import renderer_scene as RS
    f = S.load_g23()
    c2ws, intr = _cu(f["c2ws"]), _cu(f["intrinsics"])
    r = RS.NVDiffRendererScene(device="cuda", latlong_map=torch.from_numpy(f["latlong3"]), cubemap=torch.from_numpy(f["cubemap3"]))
    every = r.perspective_rendering(c2ws, intr, (8, 12), render_cubemap=True, render_uv=True, render_latlong_map=True)
    assert sorted(every) == list(f["keys_all_flags"])
    assert np.array_equal(_np(every["rays_o"]), f["rays_o"]), "rays_o: the eye, exact"
    for flags, keys in ((dict(), ["rays_d"]), (dict(render_cubemap=True), ["rays_d", "cubemap_attr"]), (dict(render_uv=True), ["rays_d", "uv"]),
                        (dict(render_uv=True, render_latlong_map=True), ["rays_d", "uv", "latlong_map_attr"])):
        one = r.perspective_rendering(c2ws, intr, (8, 12), **flags)
        assert sorted(one) == sorted(keys + ["rays_o"])
        for k in keys:
            assert torch.equal(one[k], every[k]), (flags, k)
    assert sorted(r.perspective_rendering(c2ws, intr, (8, 12), render_latlong_map=True)) == list(f["keys_latlong_without_uv"])
    direct = ops.scene_render(c2ws, intr, 8, 12, cubemap=r.cubemap, latlong=r.latlong_map, want=("rays_d", "cubemap_attr", "uv", "latlong_map_attr"))
    for k, v in direct.items():
        assert torch.equal(v, every[k]), k
    batched = r.perspective_rendering(c2ws, intr[None].expand(5, 3, 3), 8, render_cubemap=True)
    square = r.perspective_rendering(c2ws, intr, (8, 8), render_cubemap=True)
    assert torch.equal(batched["cubemap_attr"], square["cubemap_attr"]) and batched["rays_d"].shape == (5, 8, 8, 3)
    # a constant cubemap renders constant, exactly (see test_cubemap_to_latlong for why these constants)
    const = torch.tensor([0.75, 0.5, 0.25]).expand(6, 4, 4, 3).contiguous()
    c = RS.NVDiffRendererScene(device="cuda", cubemap=const).perspective_rendering(c2ws, intr, (5, 7), render_cubemap=True)["cubemap_attr"]
    assert torch.equal(c.cpu(), const[0, 0, 0].expand(5, 5, 7, 3))
    with pytest.raises(ValueError):
        RS.NVDiffRendererScene(device="cuda", cubemap=const).perspective_rendering(c2ws, intr, (5, 7), render_uv=True, render_latlong_map=True)
    # the inverse renderer: the class against the ops wrapper, and the nested flag
    img = _cu(f["images3"])
    inv = r.perspective_inverse_rendering_torch(c2ws, intr, img, (8, 12), (6, 12), render_uv=True, render_latlong_map=True)
    assert sorted(inv) == ["latlong_map_attr", "rays_d", "rays_o", "uv", "uv_alpha"] and torch.equal(inv["rays_d"], every["rays_d"])
    w2cs = torch.linalg.inv(torch.from_numpy(f["c2ws"])).cuda().contiguous()      # the class inverts on the host, as the reference does
    uv, alpha, attr = ops.scene_bake_latlong(w2cs, _cu(np.broadcast_to(f["projections"], (5, 4, 4))), 6, 12, img)
    assert torch.equal(inv["uv"], uv) and torch.equal(inv["uv_alpha"], alpha) and torch.equal(inv["latlong_map_attr"], attr)
    assert sorted(r.perspective_inverse_rendering_torch(c2ws, intr, img, (8, 12), (6, 12), render_latlong_map=True)) == ["rays_d", "rays_o"]
    per_view = r.perspective_inverse_rendering_torch(c2ws, intr[None].expand(5, 3, 3), img, (8, 12), (6, 12), render_uv=True, render_latlong_map=True)
    assert torch.equal(per_view["latlong_map_attr"], attr), "[M,3,3] intrinsics are accepted in addition"
    # layouts on the device
    cube = _cu(f["cubemap3"])
    assert np.array_equal(_np(RS.cubemap_to_flatten(cube)), f["flatten"]) and np.array_equal(_np(RS.cubemap_to_flatten_kjl(cube)), f["flatten_kjl"])
    assert torch.equal(RS.flatten_to_cubemap(RS.cubemap_to_flatten(cube)), cube)
    pcd = _np(RS.latlong_depth_to_pcd(_cu(f["pcd_depth"])))
    assert np.abs(pcd - f["pcd_depth"] * S.texel_dirs(6, 12)).max() <= 8 * S.U * f["pcd_depth"].max()


@pytest.mark.parametrize("Cc", [3, 4])
def test_g23_against_the_reference(Cc):
    """The reference's own arrays: masks exact; everything else within the reference's fp32 rounding measured on the CPU (scene_ref.REF_ROUNDING) plus the
    counted kernel bound.  Where the two sides look up at their own coordinates the coordinate difference counts times the texel contrast D: a direction
    difference e moves the cube rule by K e, K = 2 * 2 sqrt(3) * (N / 2) * D (oracle/pbr_ref.py); a uv difference moves the wrap-linear lookup by
    (Wi du + Hi dv) D and grid_sample by (W / 2 du + H / 2 dv) D."""
    from unitex_amd.texturetools import renderer_scene as RS
    f, R = S.load_g23(), S.REF_ROUNDING
    cube, lat, img = f["cubemap%d" % Cc], f["latlong%d" % Cc], f["images%d" % Cc]
    r = RS.NVDiffRendererScene(device="cuda", latlong_map=torch.from_numpy(lat), cubemap=torch.from_numpy(cube))
    c2ws, intr = _cu(f["c2ws"]), _cu(f["intrinsics"])
    got = {k: _np(v) for k, v in r.perspective_rendering(c2ws, intr, (8, 12), render_cubemap=True, render_uv=True, render_latlong_map=True).items()}
    _, rd, bound = S.rays(f["c2ws"], f["intrinsics"], 8, 12)
    ub = S.uv_bound(rd, bound)
    assert np.array_equal(got["rays_o"], f["rays_o"])
    e_d = bound.max() + R["rays"]
    assert np.abs(got["rays_d"] - f["rays_d"]).max() <= e_d
    assert (S.circle_diff(got["uv"][..., 0], f["uv"][..., 0]) <= ub[..., 0] + R["uv"]).all() and (np.abs(got["uv"][..., 1] - f["uv"][..., 1]) <= ub[..., 1] + R["uv"]).all()
    K = 2 * 2 * np.sqrt(3.0) * (4 / 2) * (cube.max() - cube.min())
    assert np.abs(got["cubemap_attr"] - f["cubemap_attr%d" % Cc]).max() <= K * e_d + S.cube_bound(cube) + S.U
    d_lat = ((12 * (ub[..., 0] + R["uv"]) + 6 * (ub[..., 1] + R["uv"])) * (lat.max() - lat.min()))[..., None]
    # (a pixel whose u differs across the wrap is the same lookup: the texture wraps)
    assert (np.abs(got["latlong_map_attr"] - f["latlong_map_attr%d" % Cc]) <= d_lat + S.wrap_bound(lat) + S.U).all()
    assert np.abs(_np(RS.cubemap_to_latlong(_cu(cube), (6, 12))) - f["cubemap_to_latlong%d" % Cc]).max() <= S.cubemap_to_latlong_bound(cube) + R["cubemap_to_latlong"]
    inv = {k: _np(v) for k, v in r.perspective_inverse_rendering_torch(c2ws, intr, _cu(img), (8, 12), (6, 12), render_uv=True, render_latlong_map=True).items()}
    assert np.array_equal(inv["uv_alpha"], f["inv_uv_alpha"]), "masks: exact"
    uv, depth, alpha, b_uv, _ = S.bake_project(f["w2cs"], f["projections"], 6, 12)
    assert (np.abs(inv["uv"] - f["inv_uv"]) <= b_uv + R["bake_uv"] * np.maximum(1.0, np.abs(uv))).all()
    cnt = alpha.sum(0)
    unseen = cnt == 0
    assert (inv["latlong_map_attr"][unseen] == 0).all() and (f["inv_latlong_map_attr%d" % Cc][unseen] == 0).all()
    d_in = np.where(alpha[..., None], b_uv + R["bake_uv_inside"], 0.0)
    move = ((12 / 2 * d_in[..., 0] + 8 / 2 * d_in[..., 1]) * (max(img.max(), 0) - min(img.min(), 0))).max(0)
    assert (np.abs(inv["latlong_map_attr"] - f["inv_latlong_map_attr%d" % Cc]) <= (move + S.bake_bound(img, cnt) + R["bake_at_own_uv"])[..., None]).all()
