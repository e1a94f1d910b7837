"""Geometry buffers (TEST INFRASTRUCTURE ONLY): the per-pixel table that gbuffer.hip has once, restated once in numpy on oracle/pixel_ref.py, for
the atlas kernel (NVDiffRendererInverse.simple_inverse_rendering / utx_uv_gbuffer; the reference: render/nvdiffrast/renderer_base.py:352-489,
fixture G17, tests/golden/make_golden_uv_maps.py) and the screen kernel (simple_rendering / utx_screen_gbuffer; renderer_base.py:101-350, fixture
G18, tests/golden/make_golden_simple_rendering.py); alpha = coverage, dr.antialias stubbed.  tests/test_uv_maps_*.py and
tests/test_simple_rendering_*.py pin it against the fixtures and hold the kernels to it with the bounds below.

Atlas bounds (u = 2^-24, the unit roundoff of float32; none of them was taken from the code under test).  m = covered, p = the interpolated
per-vertex array, (a0*u + a1*v) + a2*w with w = (1 - u) - v:
  * mask, alpha, world_position, camera_position, z_depth: the float32 restatement (interp32, utx_interpolate's order, correctly rounded
    numpy operations) is BIT-EXACT against the fixture.  The float64 restatement differs from it by the roundings of the float32 interpolation
    alone: w carries two (each <= u, so |dw| <= 2u), each product one, each sum one: <= (3 + 2 + 2) u * amax to first order, amax = the largest
    |component| of the array; INTERP_ULPS = 8 units of u * amax covers the second-order terms.
  * The other buffers are functions of the SAME float32 p on both sides (that is what the bit-exact rows establish), so the float64 restatement
    applies the table in float64 to interp32's p, and what it measures is the reference's own rounding behind the interpolation:
      distance       sqrt(x^2 + y^2 + z^2): three roundings under the root (3u relative, halved by the root), one for the root: either side
                     is within 2.5u * d of the exact value.  DIST_ULPS = 2.5 per side (units of u * d, per texel).
      normalize      c / max(len, 1e-12): len as above (2.5u relative), one division: a component, |c / len| <= 1, is within 3.5u of the exact
                     value on either side.  UNIT_ULPS = 3.5 per side (world_normal, camera_normal, ray_direction).
      cos_ray_normal (cn.x rd.x + cn.y rd.y) + cn.z rd.z of two such unit vectors: each factor carries 3.5u RELATIVE to its component, so the inputs
                     move the sum by <= 2 * 3.5u * sum |cn_i rd_i| <= 7u (Cauchy-Schwarz, unit vectors), and three products and two sums add
                     <= 3u * sum |cn_i rd_i| <= 3u.  COS_ULPS = 10 per side.
    A kernel with the same counts is then within 2 * (per-side count) of the fixture: 5u * d, 7u and 20u.  For the two normal buffers the
    project's existing bound for a normalised interpolated normal, NORMAL_ULPS = 5 (fixture G13, oracle/video_types_ref.py), is kept.
  * End to end the per-view per-vertex arrays are recomputed by utx_transform_points / utx_camera_normals, whose fixed order replaces the
    reference's torch.matmul (order unspecified): a 4-term dot product has at most 4 roundings on either side, so a camera-space coordinate
    differs by <= 8u * S, S = sum |x_k m_k| <= SMAX (pos_smax); the interpolation is a convex combination of them (<= 8u * SMAX) evaluated twice
    with up to INTERP_ULPS each: E2E_POS_ULPS = 8 + 2 * 8 = 24 units of u * SMAX per coordinate of p.  A per-vertex camera normal is a 3-term
    product (6u * sqrt(3) of the vertex normal's length, which the normalisation divides out: 11u) normalised (2 * 3.5u): 18u per component,
    and the interpolation adds 2 * 8u on values <= 1: E2E_NRM_ULPS = 34 units of u per coordinate of p.  A perturbation dp of p moves |p| by
    <= |dp|_2 and p / |p| by <= 2 |dp|_2 / |p| (per texel, with |p| of the REFERENCE's arrays: the normals of G17 are short beside the zero one).

Screen bounds (the same u; none of them was taken from the code under test):
  * mask, alpha, world_position, camera_position, z_depth, uv, v_attr, every background form: one expression, (a0*u + a1*v) + a2*w with
    w = (1 - u) - v, correctly rounded operations in one order on both sides, then a select: BIT-EXACT.
  * map_attr: the sample coordinate is the bit-exact uv.
    'nearest' is one tap: BIT-EXACT.  'nvdiffrast' is the restated lookup of G67n, a + t (b - a) along u, then along v, in torch's elementwise
    float32 operations: BIT-EXACT.
    'bilinear' is torch's own CPU grid_sample in the fixture, and that is NOT one fixed sequence of roundings: its vectorised kernel forms the pixel
    coordinate as (g + 1) * (W / 2) - 0.5 and the compiler may contract that (and the blend) into fused multiply-adds, while torch's scalar and
    device kernels -- and this build, in the back-projection sampler that G67 pins -- write ((g + 1) * W - 1) / 2, every operation rounded.  So
    'bilinear' carries a counted bound, MAP_BOUND (map_bound below):
      coordinate  a = fl(g + 1) <= 2 is the same number on both sides.  Ours: the product a W <= 2 W rounds (<= 2 W u), the subtraction rounds
                  (<= 2 W u), the halving is exact: <= 2 W u on the pixel coordinate.  A fused a (W / 2) - 0.5 rounds once (<= W u), an unfused one
                  twice (<= 2 W u).  The two coordinates differ by <= 4 W u (and 4 H u along y); ix - floor(ix) is exact.  The bilinear
                  interpolant is continuous and piecewise linear in each coordinate with slope <= R, the range of the map's values with the zero of
                  the padding included, also where the two sides fall on different sides of a texel centre: <= 4 (W + H) u R.
      blend       per side: a weight is two differences and a product (3 u relative), a term t w one more product (4 u), and the three additions
                  round partial sums <= M = max |t| (the weights sum to 1): <= (4 + 3) u M.  Fused operations only remove roundings.  Two sides: 14 u M.
      MAP_BOUND = (14 M + 4 (W + H) R) u per map: 174 u for the 16 x 24 map and 78 u for the 8 x 8 one at M = R = 1.  The largest deviation of
      the restatement from the fixture that tests/test_simple_rendering_cpu.py prints is 12 u (map 0) and 2 u (map 1): the coordinate term, far
      from its worst case.  The kernel is bit-identical to the restatement (tests/test_simple_rendering_gpu.py asserts that too), so its deviation
      is the same.
  * world_normal, camera_normal: the project's NORMAL_ULPS = 5 u; distance, ray_direction, cos_ray_normal: the counted atlas bounds above for the
    same quantities (5 u * d, 7 u, 20 u)."""
import os

import numpy as np

from .pixel_ref import interp, len3, sample, unit

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
F32, F64 = np.float32, np.float64
U = 2.0 ** -24
ATLAS, SCREEN, VIEWS = (48, 40), (40, 56), 3          # G17's atlas (also G18's atlas raster), G18's views, the views of a camera set
SETS = ("p", "o")
MODES = ("bilinear", "nearest", "nvdiffrast")
WORLD = ("world_normal", "world_position")
PER_VIEW = ("camera_normal", "camera_position", "distance", "z_depth", "ray_direction", "cos_ray_normal")
GEOMETRY = ("z_depth", "world_normal", "camera_normal", "world_position", "camera_position", "distance", "ray_direction", "cos_ray_normal")
CHANNELS = {"z_depth": 1, "world_normal": 3, "camera_normal": 3, "world_position": 3, "camera_position": 3, "distance": 1, "ray_direction": 3,
            "cos_ray_normal": 1, "uv": 2}
FILL = {"z_depth": 0.0, "world_normal": -1.0, "camera_normal": -1.0, "world_position": -1.0, "camera_position": 0.0, "distance": 0.0,
        "ray_direction": -1.0, "cos_ray_normal": -1.0, "uv": -1.0}
UNBUILT = ("render_voxel_attr", "render_voxel_network", "render_all_point_cloud", "render_visible_point_cloud", "render_map_network")
INTERP_ULPS, DIST_ULPS, UNIT_ULPS, COS_ULPS, NORMAL_ULPS = 8, 2.5, 3.5, 10, 5
E2E_POS_ULPS, E2E_NRM_ULPS = 24, 34
_FIX = {}


def load_g17():
    return np.load(os.path.join(GOLD, "g17_uv_maps.npz"), allow_pickle=False)


def load_g18():
    """the fixture, read once and shared (the arrays are never written to)"""
    if not _FIX:
        with np.load(os.path.join(GOLD, "g18_simple_rendering.npz"), allow_pickle=False) as f:
            _FIX.update({k: f[k] for k in f.files})
        for v in _FIX.values():
            v.setflags(write=False)
    return _FIX


def interp_views(attr, rast, faces, dtype=F32):
    """attr [V,C] (one mesh) or [B,V,C] (per view), rast [B,H,W,4] or [1,H,W,4] (one raster for every view) -> [B,H,W,C] in `dtype`, zeros where empty"""
    per_view = np.asarray(attr).ndim == 3
    n = len(attr) if per_view else rast.shape[0]
    return np.stack([interp(attr[b] if per_view else attr, rast[b if rast.shape[0] > 1 else 0], faces, dtype)[0] for b in range(n)])


def background_rule(value, cov, background):
    """None leaves the value; else lerp(background, value, alpha) with alpha in {0, 1}: a select"""
    if background is None:
        return value
    return np.where(cov[..., None], value, np.broadcast_to(np.asarray(background, F32), value.shape)).astype(F32)


def table(rast, faces, v_pos=None, v_nrm=None, v_pos_cam=None, v_nrm_cam=None, clip_w=None, v_uv=None, v_attr=None, maps=(), mode="bilinear",
          background=None, dtype=F32, interp_dtype=None):
    """the per-pixel table of gbuffer.hip in the kernels' operation order: every buffer the given arrays allow, in `dtype`, plus the coverage `mask`.
    rast [B,H,W,4] is the screen form (utx_screen_gbuffer): every buffer [B,H,W,C], z_depth the interpolated clip w.  rast [H,W,4] is the atlas
    form (utx_uv_gbuffer): one raster for all views, world buffers [1,H,W,C], per-view ones [B,H,W,C], z_depth the camera-space z.
    interp_dtype (default: dtype) is the precision of the interpolation alone."""
    idt = dtype if interp_dtype is None else interp_dtype
    rast = np.asarray(rast)
    atlas = rast.ndim == 3
    cov = rast[..., 3] > 0
    sel = lambda x, fill: np.where(cov[..., None], x, dtype(fill)).astype(dtype)
    views = lambda attr: interp_views(attr, rast[None] if atlas else rast, faces, idt).astype(dtype)
    out = {"mask": cov, "alpha": cov.astype(F32)[..., None]}
    if clip_w is not None:
        out["z_depth"] = sel(views(clip_w[..., None]), 0.0)
    if v_nrm is not None:
        out["world_normal"] = sel(unit(views(v_nrm)), -1.0)
    if v_pos is not None:
        out["world_position"] = sel(views(v_pos), -1.0)
    cn = rd = None
    if v_nrm_cam is not None:
        cn = unit(views(v_nrm_cam))
        out["camera_normal"] = sel(cn, -1.0)
    if v_pos_cam is not None:
        p = views(v_pos_cam)
        d = len3(p)
        rd = unit(p, d)
        out.update(camera_position=sel(p, 0.0), distance=sel(d, 0.0), ray_direction=sel(rd, -1.0))
        if atlas:
            out["z_depth"] = sel(p[..., 2:3], 0.0)
    if cn is not None and rd is not None:
        out["cos_ray_normal"] = sel((cn[..., 0:1] * rd[..., 0:1] + cn[..., 1:2] * rd[..., 1:2]) + cn[..., 2:3] * rd[..., 2:3], -1.0)
    if v_attr is not None:
        out["v_attr"] = background_rule(views(v_attr), cov, background)
    if v_uv is not None:
        out["uv"] = sel(views(v_uv), -1.0)
        if maps:
            out["map_attr"] = background_rule(np.concatenate([sample(m, out["uv"], mode) for m in maps], -1).astype(F32), cov, background)
    return out


def fixture_buffers(f, tag):
    """the reference's buffers of one camera set, keyed as the table"""
    out = {"mask": f["mask"][..., 0] > 0, "alpha": f["alpha"], "world_normal": f["world_normal"], "world_position": f["world_position"]}
    out.update({k: f["%s_%s" % (k, tag)] for k in PER_VIEW})
    return out


def pos_smax(f, tag):
    """SMAX of the module docstring for one camera set: the largest sum |x_k m_k| of a camera-space coordinate over vertices and views"""
    c2w = f["c2ws_" + tag].astype(F64)
    Rt = np.transpose(c2w[:, :3, :3], (0, 2, 1))
    t = -np.einsum("bij,bj->bi", Rt, c2w[:, :3, 3])
    return float((np.einsum("vk,bjk->bvj", np.abs(f["verts"].astype(F64)), np.abs(Rt)) + np.abs(t)[:, None, :]).max())


def bounds(key, ref_distance, kernel_side=True, own_attrs=None):
    """absolute per-pixel bound [.., H, W, 1] (or 0.0 = bit-exact) on `key` against the fixture, whose `distance` buffer is ref_distance: the
    float64 restatement carries the reference's side of the count alone, a float32 kernel both sides; own_attrs = (G17, camera set) adds the
    atlas end-to-end terms (module docstring)"""
    sides = 2.0 if kernel_side else 1.0
    b = 0.0
    if key in ("world_normal", "camera_normal"):
        b = (NORMAL_ULPS if kernel_side else UNIT_ULPS) * U
    elif key == "ray_direction":
        b = sides * UNIT_ULPS * U
    elif key == "distance":
        b = sides * DIST_ULPS * U * ref_distance.astype(F64)
    elif key == "cos_ray_normal":
        b = sides * COS_ULPS * U
    if own_attrs is not None and key in PER_VIEW:
        f, tag = own_attrs
        dpos = np.sqrt(3.0) * E2E_POS_ULPS * U * pos_smax(f, tag)                      # |dp|_2 of the camera-space position
        dist = np.maximum(ref_distance.astype(F64), 1e-30)
        drd = 2.0 * dpos / dist
        plen = np.stack([len3(interp(a, f["rast"], f["faces"], F64)[0]) for a in f["v_nrm_cam_" + tag]])
        dcn = 2.0 * np.sqrt(3.0) * E2E_NRM_ULPS * U / np.maximum(plen, 1e-30)
        b = b + {"camera_position": dpos / np.sqrt(3.0), "z_depth": dpos / np.sqrt(3.0), "distance": dpos, "ray_direction": drd, "camera_normal": dcn,
                 "cos_ray_normal": drd + dcn}[key]
    return b


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


def v_uv(f):
    return f["uvs"] * F32(2.0) - F32(1.0)


def background_cases(f, tag):
    """(fixture key, table keyword arguments, buffer) of every stored background form of G18"""
    a = f["v_attr"]
    return (("v_attr1_" + tag, dict(v_attr=a[:, :1]), "v_attr"),
            ("v_attr4_" + tag, dict(v_attr=a[:, :4]), "v_attr"),
            ("v_attr4_float_" + tag, dict(v_attr=a[:, :4], background=float(f["bg_float"])), "v_attr"),
            ("v_attr7_vec_" + tag, dict(v_attr=a, background=f["bg_vec_7"]), "v_attr"),
            ("v_attr4_dense_" + tag, dict(v_attr=a[:, :4], background=f["bg_dense_4"]), "v_attr"),
            ("map_0_bilinear_vec_" + tag, dict(v_uv=v_uv(f), maps=(f["map_0"],), background=f["bg_vec_3"]), "map_attr"),
            ("map_1_nearest_dense_" + tag, dict(v_uv=v_uv(f), maps=(f["map_1"],), mode="nearest", background=f["bg_dense_5"]), "map_attr"))


def check(name, got, ref, bound, cov):
    """prints the largest deviation (and its share of the bound) before asserting; background texels are always held to equality"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, "%s: %s %s against %s %s" % (name, got.shape, got.dtype, ref.shape, ref.dtype)
    assert np.isfinite(got).all(), name
    d = np.abs(got.astype(F64) - ref.astype(F64))
    m = np.broadcast_to(cov[..., None], d.shape)
    assert np.array_equal(got[~m], ref[~m]), "%s: background" % name
    if isinstance(bound, float) and bound == 0.0:
        print("%s: max|diff| %.3g (bit-exact required)" % (name, d.max()))
        assert got.tobytes() == ref.tobytes(), "%s: not bit-exact, max|diff| %.3g" % (name, d.max())
        return 0.0
    bb = np.broadcast_to(np.asarray(bound, F64), d.shape)
    share = float((d[m] / bb[m]).max())
    print("%s: max|diff| %.3g = %.3g u, at most %.3f of the bound" % (name, d[m].max(), d[m].max() / U, share))
    assert share <= 1.0, "%s: max|diff| %.3g is %.3f of its bound" % (name, d[m].max(), share)
    return float(d[m].max())

