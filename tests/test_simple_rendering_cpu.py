"""Screen-space buffers (NVDiffRendererInverse.simple_rendering / utx_screen_gbuffer), CPU side: the table of the reference's simple_rendering
(render/nvdiffrast/renderer_base.py:101-350) restated in numpy, in the kernel's operation order, against the reference's own buffers (fixture
G18, tests/golden/make_golden_simple_rendering.py; alpha = coverage, dr.antialias stubbed).  The GPU module (tests/test_simple_rendering_gpu.py)
uses the restatement and the bounds of this module.

Bounds (u = 2^-24; none of them was taken from the code under test):
  * mask, alpha, world_position, camera_position, z_depth, uv, v_attr, every background form: one expression, (a0*u + a1*v) + a2*w with
    w = (1 - u) - v, correctly rounded operations in one order on both sides, then a select: BIT-EXACT.
  * map_attr: the sample coordinate is the bit-exact uv.
    'nearest' is one tap: BIT-EXACT.  'nvdiffrast' is the restated lookup of G67n, a + t (b - a) along u, then along v, in torch's elementwise
    float32 operations: BIT-EXACT.
    'bilinear' is torch's own CPU grid_sample in the fixture, and that is NOT one fixed sequence of roundings: its vectorised kernel forms the pixel
    coordinate as (g + 1) * (W / 2) - 0.5 and the compiler may contract that (and the blend) into fused multiply-adds, while torch's scalar and
    device kernels -- and this build, in the back-projection sampler that G67 pins -- write ((g + 1) * W - 1) / 2, every operation rounded.  So
    'bilinear' carries a counted bound, MAP_BOUND below:
      coordinate  a = fl(g + 1) <= 2 is the same number on both sides.  Ours: the product a W <= 2 W rounds (<= 2 W u), the subtraction rounds
                  (<= 2 W u), the halving is exact: <= 2 W u on the pixel coordinate.  A fused a (W / 2) - 0.5 rounds once (<= W u), an unfused one
                  twice (<= 2 W u).  The two coordinates differ by <= 4 W u (and 4 H u along y); ix - floor(ix) is exact.  The bilinear
                  interpolant is continuous and piecewise linear in each coordinate with slope <= R, the range of the map's values with the zero of
                  the padding included, also where the two sides fall on different sides of a texel centre: <= 4 (W + H) u R.
      blend       per side: a weight is two differences and a product (3 u relative), a term t w one more product (4 u), and the three additions
                  round partial sums <= M = max |t| (the weights sum to 1): <= (4 + 3) u M.  Fused operations only remove roundings.  Two sides: 14 u M.
      MAP_BOUND = (14 M + 4 (W + H) R) u per map: 174 u for the 16 x 24 map and 78 u for the 8 x 8 one at M = R = 1.  The largest deviation of
      the restatement from the fixture that this module prints is 12 u (map 0) and 2 u (map 1): the coordinate term, far from its worst case.
      The kernel is bit-identical to the restatement (tests/test_simple_rendering_gpu.py asserts that too), so its deviation is the same.
  * world_normal, camera_normal: the project's NORMAL_ULPS = 5 u; distance, ray_direction, cos_ray_normal: the counted bounds of
    tests/test_uv_maps_cpu.py for the same quantities (5 u * d, 7 u, 20 u), whose derivation is in that module's docstring."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import test_uv_maps_cpu as UC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
U = 2.0 ** -24
H, W, B = 40, 56, 3
ATLAS = (48, 40)
SETS = ("p", "o")
MODES = ("bilinear", "nearest", "nvdiffrast")
GEOMETRY = ("z_depth", "world_normal", "camera_normal", "world_position", "camera_position", "distance", "ray_direction", "cos_ray_normal")
CHANNELS = {"z_depth": 1, "world_normal": 3, "camera_normal": 3, "world_position": 3, "camera_position": 3, "distance": 1, "ray_direction": 3,
            "cos_ray_normal": 1, "uv": 2}
FILL = {"z_depth": 0.0, "world_normal": -1.0, "camera_normal": -1.0, "world_position": -1.0, "camera_position": 0.0, "distance": 0.0,
        "ray_direction": -1.0, "cos_ray_normal": -1.0, "uv": -1.0}
EXACT = ("z_depth", "world_position", "camera_position", "uv")
UNBUILT = ("render_voxel_attr", "render_voxel_network", "render_all_point_cloud", "render_visible_point_cloud", "render_map_network")
_FIX = {}


def load():
    """the fixture, read once and shared (the arrays are never written to)"""
    if not _FIX:
        with np.load(os.path.join(GOLD, "g18_simple_rendering.npz"), allow_pickle=False) as f:
            _FIX.update({k: f[k] for k in f.files})
        for v in _FIX.values():
            v.setflags(write=False)
    return _FIX


def interp_views(attr, rast, faces):
    """attr [V,C] (one mesh) or [B,V,C] (per view), rast [B,H,W,4] -> [B,H,W,C] float32, zeros where empty"""
    per_view = np.asarray(attr).ndim == 3
    return np.stack([UC.interp(attr[b] if per_view else attr, rast[b], faces)[0] for b in range(rast.shape[0])])


def _unnormalize(g, size):
    return ((g + F32(1.0)) * F32(size) - F32(1.0)) * F32(0.5)


def sample(tex, uv, mode):
    """one map [Ht,Wt,C] at uv [...,2] in [-1,1], float32 in the kernel's order"""
    Ht, Wt, _ = tex.shape
    gx, gy = uv[..., 0], uv[..., 1]

    def tap(y, x, zero_outside=True):
        inside = (x >= 0) & (x < Wt) & (y >= 0) & (y < Ht)
        assert zero_outside or inside.all()
        t = tex[np.clip(y, 0, Ht - 1).astype(np.int64), np.clip(x, 0, Wt - 1).astype(np.int64)]
        return np.where(inside[..., None], t, F32(0.0))
    if mode in ("bilinear", "nearest"):
        ix, iy = _unnormalize(gx, Wt), _unnormalize(gy, Ht)
        if mode == "nearest":
            return tap(np.rint(iy), np.rint(ix))      # halves to even
        x0, y0 = np.floor(ix), np.floor(iy)
        tx, ty = (ix - x0)[..., None], (iy - y0)[..., None]
        w = ((F32(1.0) - tx) * (F32(1.0) - ty), tx * (F32(1.0) - ty), (F32(1.0) - tx) * ty, tx * ty)
        return ((tap(y0, x0) * w[0] + tap(y0, x0 + 1) * w[1]) + tap(y0 + 1, x0) * w[2]) + tap(y0 + 1, x0 + 1) * w[3]
    assert mode == "nvdiffrast"
    su, sv = gx * F32(0.5) + F32(0.5), gy * F32(0.5) + F32(0.5)
    su, sv = su - np.floor(su), sv - np.floor(sv)
    su, sv = su * F32(Wt) - F32(0.5), sv * F32(Ht) - F32(0.5)
    x0, y0 = np.floor(su), np.floor(sv)
    fu, fv = (su - x0)[..., None], (sv - y0)[..., None]
    x1, y1 = x0 + 1, y0 + 1
    x0, y0, x1, y1 = np.where(x0 < 0, x0 + Wt, x0), np.where(y0 < 0, y0 + Ht, y0), np.where(x1 >= Wt, x1 - Wt, x1), np.where(y1 >= Ht, y1 - Ht, y1)
    lerp = lambda a, b, t: a + (b - a) * t
    return lerp(lerp(tap(y0, x0, False), tap(y0, x1, False), fu), lerp(tap(y1, x0, False), tap(y1, x1, False), fu), fv)


def background_rule(value, cov, background):
    """None leaves the value; else lerp(background, value, alpha) with alpha in {0, 1}: a select"""
    if background is None:
        return value
    return np.where(cov[..., None], value, np.broadcast_to(np.asarray(background, F32), value.shape)).astype(F32)


def table(rast, faces, v_pos=None, v_nrm=None, clip_w=None, v_pos_cam=None, v_nrm_cam=None, v_uv=None, v_attr=None, maps=(), mode="bilinear",
          background=None):
    """the table of utx_screen_gbuffer in the kernel's operation order: every buffer the given arrays allow, [B,H,W,C] float32, mask [B,H,W] bool"""
    cov = np.asarray(rast)[..., 3] > 0
    sel = lambda x, fill: np.where(cov[..., None], x, F32(fill)).astype(F32)
    out = {"mask": cov, "alpha": cov.astype(F32)[..., None]}
    if clip_w is not None:
        out["z_depth"] = sel(interp_views(clip_w[..., None], rast, faces), 0.0)
    if v_nrm is not None:
        out["world_normal"] = sel(UC._unit(interp_views(v_nrm, rast, faces)), -1.0)
    if v_pos is not None:
        out["world_position"] = sel(interp_views(v_pos, rast, faces), -1.0)
    cn = rd = None
    if v_nrm_cam is not None:
        cn = UC._unit(interp_views(v_nrm_cam, rast, faces))
        out["camera_normal"] = sel(cn, -1.0)
    if v_pos_cam is not None:
        p = interp_views(v_pos_cam, rast, faces)
        d = UC._len3(p)
        rd = UC._unit(p, d)
        out.update(camera_position=sel(p, 0.0), distance=sel(d, 0.0), ray_direction=sel(rd, -1.0))
    if cn is not None and rd is not None:
        out["cos_ray_normal"] = sel((cn[..., 0:1] * rd[..., 0:1] + cn[..., 1:2] * rd[..., 1:2]) + cn[..., 2:3] * rd[..., 2:3], -1.0)
    if v_attr is not None:
        out["v_attr"] = background_rule(interp_views(v_attr, rast, faces), cov, background)
    if v_uv is not None:
        out["uv"] = sel(interp_views(v_uv, rast, faces), -1.0)
        if maps:
            out["map_attr"] = background_rule(np.concatenate([sample(m, out["uv"], mode) for m in maps], -1).astype(F32), cov, background)
    return out


def bounds(key, ref_distance):
    """absolute bound (0.0 = bit-exact) of a float32 evaluation in the kernel's order against the fixture (module docstring)"""
    if key in ("world_normal", "camera_normal"):
        return UC.NORMAL_ULPS * U
    if key == "ray_direction":
        return 2 * UC.UNIT_ULPS * U
    if key == "distance":
        return 2 * UC.DIST_ULPS * U * ref_distance.astype(F64)
    if key == "cos_ray_normal":
        return 2 * UC.COS_ULPS * U
    return 0.0


def map_bound(mode, maps):
    """per-channel absolute bound [sum C_i] of map_attr against the fixture (0.0: bit-exact); module docstring"""
    if mode != "bilinear":
        return 0.0
    per_map = []
    for m in maps:
        M = float(np.abs(m).max())
        R = max(float(m.max()), 0.0) - min(float(m.min()), 0.0)
        per_map.append(np.full(m.shape[2], (14.0 * M + 4.0 * (m.shape[0] + m.shape[1]) * R) * U))
    return np.concatenate(per_map)


def check(name, got, ref, bound, cov):
    """UC.check over a batch of views (its coverage is [B,H,W] here as well)"""
    return UC.check(name, got, ref, bound, cov)


def v_uv(f):
    return f["uvs"] * F32(2.0) - F32(1.0)


def background_cases(f, tag):
    """(fixture key, table keyword arguments, buffer) of every stored background form"""
    a = f["v_attr"]
    return (("v_attr1_" + tag, dict(v_attr=a[:, :1]), "v_attr"),
            ("v_attr4_" + tag, dict(v_attr=a[:, :4]), "v_attr"),
            ("v_attr4_float_" + tag, dict(v_attr=a[:, :4], background=float(f["bg_float"])), "v_attr"),
            ("v_attr7_vec_" + tag, dict(v_attr=a, background=f["bg_vec_7"]), "v_attr"),
            ("v_attr4_dense_" + tag, dict(v_attr=a[:, :4], background=f["bg_dense_4"]), "v_attr"),
            ("map_0_bilinear_vec_" + tag, dict(v_uv=v_uv(f), maps=(f["map_0"],), background=f["bg_vec_3"]), "map_attr"),
            ("map_1_nearest_dense_" + tag, dict(v_uv=v_uv(f), maps=(f["map_1"],), mode="nearest", background=f["bg_dense_5"]), "map_attr"))


def test_fixture_is_what_the_issue_asks_for():
    f = load()
    assert os.path.getsize(os.path.join(GOLD, "g18_simple_rendering.npz")) < 1024 * 1024
    V = f["verts"].shape[0]
    assert H != W and f["uvs"].shape == (V, 2) and f["v_nrm"].shape == (V, 3) and f["v_attr"].shape == (V, 7) and f["faces"].max() == V - 1
    assert f["map_0"].shape == (16, 24, 3) and f["map_1"].shape == (8, 8, 5)
    assert (f["uvs"].min(0) == 0).all() and (f["uvs"].max(0) == 1).all()
    ln = np.linalg.norm(f["v_nrm"].astype(F64), axis=-1)
    assert (ln == 0).sum() == 1 and ln[ln > 0].min() < 0.6 and ln.max() > 1.8
    for tag in SETS:
        assert f["c2ws_" + tag].shape == (B, 4, 4) and f["intr_" + tag].shape[-2:] == (3, 3)
        assert f["rast_" + tag].shape == (B, H, W, 4) and f["clip_w_" + tag].shape == (B, V)
        assert f["v_pos_cam_" + tag].shape == f["v_nrm_cam_" + tag].shape == (B, V, 3)
        cov = f["rast_" + tag][..., 3] > 0
        assert cov.reshape(B, -1).any(1).all() and not cov.reshape(B, -1).all(1).any()
        for k, ch in CHANNELS.items():
            assert f["%s_%s" % (k, tag)].shape == (B, H, W, ch), k
            assert (f["%s_%s" % (k, tag)][~cov] == FILL[k]).all(), k
        for i, ch in ((0, 3), (1, 5)):
            for mode in MODES:
                assert f["map_%d_%s_%s" % (i, mode, tag)].shape == (B, H, W, ch)
        # zero padding and wrap disagree somewhere, and nearest differs from both
        assert not np.array_equal(f["map_0_bilinear_" + tag], f["map_0_nvdiffrast_" + tag])
        assert not np.array_equal(f["map_0_bilinear_" + tag], f["map_0_nearest_" + tag])
    assert not np.array_equal(f["c2ws_p"], f["c2ws_o"]) and not np.array_equal(f["clip_w_p"], f["clip_w_o"])
    assert (f["clip_w_o"] == 1).all() and not (f["clip_w_p"] == 1).any()          # orthographic: w = 1; perspective: the camera depth
    assert f["atlas_rast"].shape == ATLAS + (4,) and f["atlas_v_attr4_half"].shape == (1,) + ATLAS + (4,)
    # the readings about the flags that stay unbuilt: the reference's own calls raise
    for name in ("voxel_attr", "all_point_cloud", "visible_point_cloud"):
        assert str(f["refusal_" + name]) == "RuntimeError", (name, str(f["refusal_" + name]))
    assert all(np.isfinite(v).all() for v in f.values() if v.dtype == F32)


@pytest.mark.parametrize("tag", SETS)
def test_border_taps_and_exact_halves(tag):
    """per mode and map at least one covered pixel has a tap outside the map, and at least one 'nearest' pixel lies on an exact half"""
    f = load()
    uv, cov = f["uv_" + tag], f["rast_" + tag][..., 3] > 0
    for m in (f["map_0"], f["map_1"]):
        Ht, Wt, _ = m.shape
        ix, iy = _unnormalize(uv[..., 0], Wt), _unnormalize(uv[..., 1], Ht)
        x0, y0 = np.floor(ix), np.floor(iy)
        assert (cov & ((x0 < 0) | (x0 + 1 >= Wt) | (y0 < 0) | (y0 + 1 >= Ht))).any(), "bilinear"
        nx, ny = np.rint(ix), np.rint(iy)
        assert (cov & ((nx < 0) | (nx >= Wt) | (ny < 0) | (ny >= Ht))).any(), "nearest"
        su = uv[..., 0] * F32(0.5) + F32(0.5)
        su = (su - np.floor(su)) * F32(Wt) - F32(0.5)
        assert (cov & ((np.floor(su) < 0) | (np.floor(su) + 1 >= Wt))).any(), "nvdiffrast"
        # an exact half below an even index: rint goes down to even there, and rounding half up would pick the next texel, which is inside the map
        half_x, half_y = cov & (ix - x0 == 0.5) & (x0 % 2 == 0) & (x0 + 1 < Wt), cov & (iy - y0 == 0.5) & (y0 % 2 == 0) & (y0 + 1 < Ht)
        assert half_x.any() or half_y.any()
        assert (nx[half_x] == x0[half_x]).all() and (ny[half_y] == y0[half_y]).all()
    tri = f["faces"][f["nudged_faces"]]
    assert (f["uvs"][tri[0]] == 0.125).all() and (f["uvs"][tri[1], 0] == 1.0).all()


@pytest.mark.parametrize("tag", SETS)
def test_restatement_reproduces_the_fixture(tag):
    f = load()
    rast, faces = f["rast_" + tag], f["faces"]
    cov = rast[..., 3] > 0
    got = table(rast, faces, f["verts"], f["v_nrm"], f["clip_w_" + tag], f["v_pos_cam_" + tag], f["v_nrm_cam_" + tag], v_uv(f))
    for k in GEOMETRY + ("uv",):
        check("%s %s" % (k, tag), got[k], f["%s_%s" % (k, tag)], bounds(k, f["distance_" + tag]), cov)
    for mode in MODES:
        single = []
        for i in range(2):
            one = table(rast, faces, v_uv=v_uv(f), maps=(f["map_%d" % i],), mode=mode)["map_attr"]
            check("map_%d %s %s" % (i, mode, tag), one, f["map_%d_%s_%s" % (i, mode, tag)], map_bound(mode, (f["map_%d" % i],)), cov)
            single.append(one)
        both = table(rast, faces, v_uv=v_uv(f), maps=(f["map_0"], f["map_1"]), mode=mode)["map_attr"]
        assert both.tobytes() == np.concatenate(single, -1).tobytes()
    for key, kw, buf in background_cases(f, tag):
        check(key, table(rast, faces, **kw)[buf], f[key], map_bound(kw.get("mode", "bilinear"), kw["maps"]) if buf == "map_attr" else 0.0, cov)


def test_atlas_v_attr_restatement():
    f = load()
    got = table(f["atlas_rast"][None], f["faces"], v_attr=f["v_attr"][:, :4], background=0.5)["v_attr"]
    cov = f["atlas_rast"][None][..., 3] > 0
    check("atlas v_attr", got, f["atlas_v_attr4_half"], 0.0, cov)
    assert (got[~cov] == 0.5).all() and cov.any() and not cov.all()


def test_abi_binds_the_screen_gbuffer_entry_point():
    import ctypes as C
    from unitex_amd import _lib
    from unitex_amd.texturetools import ops
    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "unitex_hip.h")).read()
    assert "utx_screen_gbuffer" in _lib.SYMBOLS and hasattr(lib, "utx_screen_gbuffer") and "int utx_screen_gbuffer(" in hdr
    assert len(_lib.SYMBOLS["utx_screen_gbuffer"][1]) == 26
    for name, (bit, ch) in ops.SCREEN_GBUFFERS.items():
        assert "#define UTX_SGB_%s %d\n" % (name.upper(), 1 << bit) in hdr
        assert name in ("mask", "alpha") or ch == CHANNELS.get(name)
    n = len(ops.SCREEN_GBUFFERS)
    assert "#define UTX_SGB_COUNT %d\n" % n in hdr and "#define UTX_SGB_ALL %d\n" % ((1 << n) - 1) in hdr
    assert "#define UTX_SGB_MAX_MAPS %d\n" % ops.SCREEN_MAX_MAPS in hdr
    for name, v in ops.SCREEN_FILTERS.items():
        assert "#define UTX_SGB_FILTER_%s %d\n" % (name.upper(), v) in hdr
    # the argument checks of the C entry point come before any device call, so they run here: no context, null pointers
    outs = (C.c_void_p * n)()
    assert lib.utx_screen_gbuffer(None, None, None, None, None, None, None, 0, None, None, None, 4, 1, 8, 8, 0, None, None, 0, 0, 0.0, None, None, 1, outs,
                                  None) == -2


def test_python_argument_checks_need_no_gpu(monkeypatch):
    """ValueError / NotImplementedError / TypeError / KeyError come before the library is touched"""
    import torch
    from unitex_amd.texturetools import ops
    from unitex_amd.texturetools.renderer_inverse import DeviceMesh, NVDiffRendererInverse

    def no_ctx(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "get_ctx", no_ctx)
    inv = NVDiffRendererInverse(device="cpu")
    cam = (torch.eye(4)[None], torch.eye(3)[None], (H, W))
    for flag in UNBUILT:
        with pytest.raises(NotImplementedError, match=flag):
            inv.simple_rendering(*cam, **{flag: True})
    with pytest.raises(TypeError, match="render_albedo"):
        inv.simple_rendering(*cam, render_albedo=True)
    inv.pbr_mesh = DeviceMesh.__new__(DeviceMesh)             # a mesh of five vertices that nothing else is read from
    inv.pbr_mesh.vertices = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="v_attr"):
        inv.simple_rendering(*cam, render_v_attr=True)
    with pytest.raises(ValueError, match="v_attr"):
        inv.simple_rendering(*cam, render_v_attr=True, v_attr=torch.zeros(4, 2))
    with pytest.raises(ValueError, match="map_attr"):
        inv.simple_rendering(*cam, render_uv=True, render_map_attr=True)
    with pytest.raises(ValueError, match="render_uv"):
        inv.simple_rendering(*cam, render_map_attr=True, map_attr=torch.zeros(2, 2, 1))
    with pytest.raises(ValueError, match="5 maps"):
        inv.simple_rendering(*cam, render_uv=True, render_map_attr=True, map_attr=(torch.zeros(2, 2, 1),) * 5)
    with pytest.raises(ValueError, match="grid_interpolate_mode"):
        inv.simple_rendering(*cam, grid_interpolate_mode="bicubic")
    with pytest.raises(ValueError, match="v_attr"):
        inv.simple_inverse_rendering(None, ATLAS, render_v_attr=True, v_attr=torch.zeros(4, 2))
    x = object()
    with pytest.raises(KeyError):
        ops.screen_gbuffer(x, x, x, want=("mask", "voxel_attr"))
    with pytest.raises(ValueError):
        ops.screen_gbuffer(x, x, x, want=())
    with pytest.raises(ValueError):
        ops.screen_gbuffer(x, x, x, want=("mask", "distance"))
    with pytest.raises(ValueError):
        ops.screen_gbuffer(x, x, x, want=("z_depth",))
    with pytest.raises(ValueError):
        ops.screen_gbuffer(x, x, x, want=("mask",), filter="bicubic")


def test_generator_reproduces_committed_fixture(tmp_path):
    """re-runs tests/golden/make_golden_simple_rendering.py and compares every array bit for bit.  The generator imports the reference's own
    Python, which lives outside this repository (make_golden.REF): the test runs wherever that tree is present and skips, before doing any
    work, where it is not (e.g. a GPU box that holds the repository alone)."""
    sys.path.insert(0, GOLD)
    try:
        from make_golden import REF
    finally:
        sys.path.remove(GOLD)
    if not os.path.isdir(REF):
        pytest.skip("the reference tree is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_simple_rendering.py"), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    new, old = np.load(str(tmp_path / "g18_simple_rendering.npz")), load()
    assert sorted(new.files) == sorted(old)
    for k in old:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), k
