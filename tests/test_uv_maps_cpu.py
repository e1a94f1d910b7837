"""Atlas-space geometry buffers (NVDiffRendererInverse.simple_inverse_rendering / utx_uv_gbuffer), CPU side: the table of the reference's
simple_inverse_rendering (render/nvdiffrast/renderer_base.py:352-489) restated in numpy against the reference's own buffers (fixture G17,
tests/golden/make_golden_uv_maps.py; alpha = coverage, dr.antialias stubbed).  The restatement (the atlas form of table) and the bounds, with
their derivation, are in oracle/gbuffer_ref.py; the GPU module (tests/test_uv_maps_gpu.py) uses them too."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.gbuffer_ref import ATLAS, CHANNELS, INTERP_ULPS, PER_VIEW, SETS, VIEWS, WORLD, F32, F64, U, bounds, check, fixture_buffers, table
from oracle.gbuffer_ref import load_g17 as load

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(H, W), B = ATLAS, VIEWS
EXACT = ("world_position", "camera_position", "z_depth")


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
        check("%s %s float32" % (k, tag), got[k], ref[k], bounds(k, ref["distance"]), ref["mask"])


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
        bb = np.broadcast_to(np.asarray(bounds(k, ref["distance"], kernel_side=False), F64), d.shape)
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
