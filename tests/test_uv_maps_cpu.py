"""Atlas-space geometry buffers (NVDiffRendererInverse.simple_inverse_rendering / utx_uv_gbuffer), CPU side: the table of the reference's
simple_inverse_rendering (render/nvdiffrast/renderer_base.py:352-489) restated in numpy against the reference's own buffers (fixture G17,
tests/golden/make_golden_uv_maps.py; alpha = coverage, dr.antialias stubbed).  The GPU module (tests/test_uv_maps_gpu.py) uses the
restatement and the bounds of this module.

Bounds (u = 2^-24, the unit roundoff of float32; none of them was taken from the code under test).  m = covered, p = the interpolated
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
    project's existing bound for a normalised interpolated normal, NORMAL_ULPS = 5 (fixture G13, tests/test_video_types_cpu.py), is kept.
  * End to end the per-view per-vertex arrays are recomputed by utx_transform_points / utx_camera_normals, whose fixed order replaces the
    reference's torch.matmul (order unspecified): a 4-term dot product has at most 4 roundings on either side, so a camera-space coordinate
    differs by <= 8u * S, S = sum |x_k m_k| <= SMAX (pos_smax); the interpolation is a convex combination of them (<= 8u * SMAX) evaluated twice
    with up to INTERP_ULPS each: E2E_POS_ULPS = 8 + 2 * 8 = 24 units of u * SMAX per coordinate of p.  A per-vertex camera normal is a 3-term
    product (6u * sqrt(3) of the vertex normal's length, which the normalisation divides out: 11u) normalised (2 * 3.5u): 18u per component,
    and the interpolation adds 2 * 8u on values <= 1: E2E_NRM_ULPS = 34 units of u per coordinate of p.  A perturbation dp of p moves |p| by
    <= |dp|_2 and p / |p| by <= 2 |dp|_2 / |p| (per texel, with |p| of the REFERENCE's arrays: the normals of G17 are short beside the zero one)."""
import os
import subprocess
import sys

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
U = 2.0 ** -24
H, W, B = 48, 40, 3
SETS = ("p", "o")
WORLD = ("world_normal", "world_position")
PER_VIEW = ("camera_normal", "camera_position", "distance", "z_depth", "ray_direction", "cos_ray_normal")
CHANNELS = {"world_normal": 3, "world_position": 3, "camera_normal": 3, "camera_position": 3, "distance": 1, "z_depth": 1, "ray_direction": 3,
            "cos_ray_normal": 1}
FILL = {"world_normal": -1.0, "world_position": -1.0, "camera_normal": -1.0, "camera_position": 0.0, "distance": 0.0, "z_depth": 0.0,
        "ray_direction": -1.0, "cos_ray_normal": -1.0}
EXACT = ("world_position", "camera_position", "z_depth")
INTERP_ULPS, DIST_ULPS, UNIT_ULPS, COS_ULPS, NORMAL_ULPS = 8, 2.5, 3.5, 10, 5
E2E_POS_ULPS, E2E_NRM_ULPS = 24, 34


def load():
    return np.load(os.path.join(GOLD, "g17_uv_maps.npz"), allow_pickle=False)


def interp(attr, rast, faces, dtype=F32):
    """utx_interpolate: (a0*u + a1*v) + a2*((1-u)-v) in `dtype`, zeros where empty; attr [V,C] -> ([H,W,C], coverage [H,W])"""
    attr, r = np.asarray(attr, dtype), np.asarray(rast, F32)
    tid = r[..., 3].astype(np.int64) - 1
    cov = tid >= 0
    f = np.asarray(faces)[np.where(cov, tid, 0)]
    u, v = r[..., 0:1].astype(dtype), r[..., 1:2].astype(dtype)
    w = (dtype(1.0) - u) - v
    out = (attr[f[..., 0]] * u + attr[f[..., 1]] * v) + attr[f[..., 2]] * w
    return np.where(cov[..., None], out, dtype(0.0)).astype(dtype), cov


def _len3(p):
    return np.sqrt((p[..., 0:1] * p[..., 0:1] + p[..., 1:2] * p[..., 1:2]) + p[..., 2:3] * p[..., 2:3])


def _unit(p, length=None):
    return p / np.maximum(_len3(p) if length is None else length, p.dtype.type(1e-12))


def table(rast, faces, v_pos=None, v_nrm=None, v_pos_cam=None, v_nrm_cam=None, dtype=F32, interp_dtype=None):
    """the table of utx_uv_gbuffer in the kernel's operation order: every buffer the given arrays allow, [1 | B,H,W,C] of `dtype`, plus
    mask [H,W] bool.  interp_dtype (default: dtype) is the precision of the interpolation alone."""
    idt = dtype if interp_dtype is None else interp_dtype
    cov = np.asarray(rast)[..., 3] > 0
    sel = lambda x, fill: np.where(cov[..., None], x, dtype(fill)).astype(dtype)
    out = {"mask": cov, "alpha": cov.astype(F32)[..., None]}
    if v_nrm is not None:
        out["world_normal"] = sel(_unit(interp(v_nrm, rast, faces, idt)[0].astype(dtype)), -1.0)[None]
    if v_pos is not None:
        out["world_position"] = sel(interp(v_pos, rast, faces, idt)[0].astype(dtype), -1.0)[None]
    cn = rd = None
    if v_nrm_cam is not None:
        cn = np.stack([_unit(interp(a, rast, faces, idt)[0].astype(dtype)) for a in v_nrm_cam])
        out["camera_normal"] = sel(cn, -1.0)
    if v_pos_cam is not None:
        p = np.stack([interp(a, rast, faces, idt)[0].astype(dtype) for a in v_pos_cam])
        d = _len3(p)
        rd = _unit(p, d)
        out.update(camera_position=sel(p, 0.0), distance=sel(d, 0.0), z_depth=sel(p[..., 2:3], 0.0), ray_direction=sel(rd, -1.0))
    if cn is not None and rd is not None:
        out["cos_ray_normal"] = sel((cn[..., 0:1] * rd[..., 0:1] + cn[..., 1:2] * rd[..., 1:2]) + cn[..., 2:3] * rd[..., 2:3], -1.0)
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


def bounds(f, tag, key, ref, kernel_side=True, own_attrs=False):
    """absolute per-texel bound [.., H, W, 1] (or 0.0 = bit-exact) on `key` against the fixture `ref` dict: the float64 restatement carries
    the reference's side of the count alone, a float32 kernel both sides; own_attrs adds the end-to-end terms (module docstring)"""
    sides = 2.0 if kernel_side else 1.0
    b = 0.0
    if key in ("world_normal", "camera_normal"):
        b = (NORMAL_ULPS if kernel_side else UNIT_ULPS) * U
    elif key == "ray_direction":
        b = sides * UNIT_ULPS * U
    elif key == "distance":
        b = sides * DIST_ULPS * U * ref["distance"].astype(F64)
    elif key == "cos_ray_normal":
        b = sides * COS_ULPS * U
    if own_attrs and key in PER_VIEW:
        dpos = np.sqrt(3.0) * E2E_POS_ULPS * U * pos_smax(f, tag)                      # |dp|_2 of the camera-space position
        dist = np.maximum(ref["distance"].astype(F64), 1e-30)
        drd = 2.0 * dpos / dist
        plen = np.stack([_len3(interp(a, f["rast"], f["faces"], F64)[0]) for a in f["v_nrm_cam_" + tag]])
        dcn = 2.0 * np.sqrt(3.0) * E2E_NRM_ULPS * U / np.maximum(plen, 1e-30)
        b = b + {"camera_position": dpos / np.sqrt(3.0), "z_depth": dpos / np.sqrt(3.0), "distance": dpos, "ray_direction": drd, "camera_normal": dcn,
                 "cos_ray_normal": drd + dcn}[key]
    return b


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


def test_fixture_is_what_the_issue_asks_for():
    f = load()
    assert os.path.getsize(os.path.join(GOLD, "g17_uv_maps.npz")) < 512 * 1024
    keys = {"verts", "faces", "uvs", "v_nrm", "rast", "mask", "alpha", "world_normal", "world_position", "none_world_normal", "none_world_position"}
    for tag in SETS:
        keys |= {"c2ws_" + tag, "intr_" + tag, "v_pos_cam_" + tag, "v_nrm_cam_" + tag} | {"%s_%s" % (k, tag) for k in PER_VIEW}
    assert set(f.files) == keys
    assert all(f[k].dtype == (np.int32 if k == "faces" else F32) for k in f.files)
    V = f["verts"].shape[0]
    assert f["rast"].shape == (H, W, 4) and f["mask"].shape == (H, W, 1) and f["alpha"].shape == (H, W, 1) and H != W
    assert f["uvs"].shape == (V, 2) and f["v_nrm"].shape == (V, 3) and f["faces"].max() == V - 1
    for k in WORLD:
        assert f[k].shape == (1, H, W, 3) and np.array_equal(f[k], f["none_" + k])
    for tag in SETS:
        assert f["c2ws_" + tag].shape == (B, 4, 4) and f["v_pos_cam_" + tag].shape == f["v_nrm_cam_" + tag].shape == (B, V, 3)
        for k in PER_VIEW:
            assert f["%s_%s" % (k, tag)].shape == (B, H, W, CHANNELS[k]), k
    assert not np.array_equal(f["c2ws_p"], f["c2ws_o"]) and not np.array_equal(f["v_pos_cam_p"], f["v_pos_cam_o"])
    # two charts and a gutter of background texels between them; both background values occur
    cov = f["mask"][..., 0] > 0
    assert np.array_equal(cov, f["rast"][..., 3] > 0) and np.array_equal(f["alpha"], f["mask"])
    assert cov[:, :W // 2].any() and cov[:, W // 2:].any() and not cov[:, W // 2 - 1:W // 2 + 1].any()
    assert (f["world_position"][0][~cov] == -1).all() and (f["camera_position_p"][:, ~cov] == 0).all()
    # normals off unit length, one of them zero: its camera-space normal is 0 / 1e-12 = 0 in every view, and everything stays finite
    ln = np.linalg.norm(f["v_nrm"].astype(F64), axis=-1)
    assert (ln == 0).sum() == 1 and ln[ln > 0].min() < 0.6 and ln.max() > 1.8
    z = int(np.argmin(ln))
    assert (f["v_nrm_cam_p"][:, z] == 0).all() and (f["faces"] == z).any(1).sum() == 6
    assert all(np.isfinite(f[k]).all() for k in f.files)


@pytest.mark.parametrize("tag", SETS)
def test_float32_restatement_reproduces_the_interpolated_buffers_bit_for_bit(tag):
    f = load()
    got = table(f["rast"], f["faces"], f["verts"], f["v_nrm"], f["v_pos_cam_" + tag], f["v_nrm_cam_" + tag])
    ref = fixture_buffers(f, tag)
    assert np.array_equal(got["mask"], ref["mask"]) and got["alpha"].tobytes() == ref["alpha"].tobytes()
    for k in EXACT:
        check("%s %s float32" % (k, tag), got[k], ref[k], 0.0, ref["mask"])
    for k in ("world_normal", "camera_normal", "distance", "ray_direction", "cos_ray_normal"):       # a float32 evaluation: both sides of the count
        check("%s %s float32" % (k, tag), got[k], ref[k], bounds(f, tag, k, ref), ref["mask"])


@pytest.mark.parametrize("tag", SETS)
def test_float64_restatement_reproduces_reference_buffers(tag):
    """float64 throughout for the pure interpolations (held to the float32 rounding of the interpolation), float64 behind the float32
    interpolation for the rest: the recorded maxima are the reference's own rounding (DESIGN.md section 8 quotes them)"""
    f = load()
    ref = fixture_buffers(f, tag)
    arrays = (f["verts"], f["v_nrm"], f["v_pos_cam_" + tag], f["v_nrm_cam_" + tag])
    full = table(f["rast"], f["faces"], *arrays, dtype=F64)
    assert np.array_equal(full["mask"], ref["mask"]) and np.array_equal(full["alpha"], ref["alpha"])
    for k, amax in (("world_position", np.abs(f["verts"]).max()), ("camera_position", np.abs(f["v_pos_cam_" + tag]).max()),
                    ("z_depth", np.abs(f["v_pos_cam_" + tag][..., 2]).max())):
        check("%s %s float64" % (k, tag), full[k].astype(F32), ref[k], INTERP_ULPS * U * float(amax), ref["mask"])
    behind = table(f["rast"], f["faces"], *arrays, dtype=F64, interp_dtype=F32)
    for k in ("world_normal", "camera_normal", "distance", "ray_direction", "cos_ray_normal"):
        # compared in float64: rounding the restatement to float32 would add half an ulp that is nobody's error
        d = np.abs(behind[k] - ref[k].astype(F64))
        bb = np.broadcast_to(np.asarray(bounds(f, tag, k, ref, kernel_side=False), F64), d.shape)
        m = np.broadcast_to(ref["mask"][..., None], d.shape)
        print("%s %s float64 behind the interpolation: max|diff| %.3g = %.3g u, at most %.3f of the reference's side of the bound" %
              (k, tag, d[m].max(), d[m].max() / U, (d[m] / bb[m]).max()))
        assert (d[m] <= bb[m]).all() and np.array_equal(behind[k][~m], ref[k].astype(F64)[~m]), k


def test_abi_binds_the_uv_gbuffer_entry_point():
    from unitex_amd import _lib
    from unitex_amd.texturetools import ops
    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "unitex_hip.h")).read()
    assert "utx_uv_gbuffer" in _lib.SYMBOLS and hasattr(lib, "utx_uv_gbuffer") and "int utx_uv_gbuffer(" in hdr
    assert len(_lib.SYMBOLS["utx_uv_gbuffer"][1]) == 14
    for name, (bit, ch, per) in ops.UV_GBUFFERS.items():
        assert "#define UTX_UVGB_%s %d\n" % (name.upper(), 1 << bit) in hdr
        assert name in ("mask", "alpha") or (CHANNELS[name] == ch and per == (name in PER_VIEW))
    assert "#define UTX_UVGB_COUNT %d\n" % len(ops.UV_GBUFFERS) in hdr and "#define UTX_UVGB_ALL %d\n" % ((1 << len(ops.UV_GBUFFERS)) - 1) in hdr
    # the argument checks of the C entry point come before any device call, so they run here: no context, null pointers
    import ctypes as C
    outs = (C.c_void_p * 10)()
    assert lib.utx_uv_gbuffer(None, None, None, None, None, None, None, 4, 0, 8, 8, 1, outs, None) == -2


def test_python_argument_checks_need_no_gpu(monkeypatch):
    """ValueError / NotImplementedError / TypeError come before the library is touched: get_ctx is replaced by a stub that fails the test if it is reached"""
    from unitex_amd.texturetools import ops
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse

    def no_ctx(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "get_ctx", no_ctx)
    inv = NVDiffRendererInverse(device="cpu")
    for flag in ("camera_normal", "camera_position", "distance", "z_depth", "ray_direction", "cos_ray_normal"):
        with pytest.raises(ValueError, match=flag):
            inv.simple_inverse_rendering(None, (H, W), **{"render_" + flag: True})
    for flag in ("render_voxel_attr", "render_v_attr", "render_uv", "render_map_attr", "render_all_point_cloud", "render_visible_point_cloud"):
        with pytest.raises(NotImplementedError, match=flag):
            inv.simple_inverse_rendering(None, (H, W), **{flag: True})
    with pytest.raises(TypeError, match="render_albedo"):
        inv.simple_inverse_rendering(None, (H, W), render_albedo=True)
    with pytest.raises(TypeError, match="intrinsics"):
        inv.simple_inverse_rendering(None, (H, W), intrinsics=None)
    x = object()
    with pytest.raises(ValueError):
        ops.uv_gbuffer(x, x, x, x, c2ws=None, want=("mask", "z_depth"))
    with pytest.raises(KeyError):
        ops.uv_gbuffer(x, x, x, x, want=("mask", "uv"))
    with pytest.raises(ValueError):
        ops.uv_gbuffer(x, x, x, x, want=())


def test_generator_reproduces_committed_fixture(tmp_path):
    """re-runs tests/golden/make_golden_uv_maps.py and compares every array bit for bit.  The generator imports the reference's own Python, which
    lives outside this repository (make_golden.REF): the test runs wherever that tree is present and skips, before doing any work, where it
    is not (e.g. a GPU box that holds the repository alone)."""
    sys.path.insert(0, GOLD)
    try:
        from make_golden import REF
    finally:
        sys.path.remove(GOLD)
    if not os.path.isdir(REF):
        pytest.skip("the reference tree is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_uv_maps.py"), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    new, old = np.load(str(tmp_path / "g17_uv_maps.npz")), load()
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), k
