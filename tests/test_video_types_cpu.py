"""Geometry-buffer video types of VideoExporter.export_orbit_video, CPU side: the numpy restatement of the reference's simple_rendering and export_video
(oracle/video_types_ref.py, which also holds the bounds and their derivation) against the reference's own frames (fixture G13,
tests/golden/make_golden_video_types.py; alpha = coverage, dr.antialias stubbed).  The GPU module (tests/test_video_types_gpu.py) uses the same
restatement at other sizes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import geom_ref as G
from oracle.video_types_ref import (CAMNRM_ULPS, GEOM_TYPES, NORMALIZE, RGB_ULPS, SETS, F32, U, check_frame, check_u8, fixture_attr, fixture_frames,
                                    float_bound, load, rgb_texture, shade, value_range, vertex_attr)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rgb_oracle_reproduces_reference_frames():
    """the seventh type: the oracle's texture_shade (bit-identical to utx_texture_shade, tests/test_geometry_gpu.py) on the fixture's rast
    against the reference's own rgb frames, both camera models"""
    f = load()
    for tag, (persp, n, size) in SETS.items():
        assert np.array_equal(f["rgb_" + tag][f["alpha_" + tag] == 0], np.ones((int((f["alpha_" + tag] == 0).sum()), 3), F32))
        for i in range(n):
            got = G.texture_shade(f["rast_" + tag][i], f["uvs"], f["faces"], rgb_texture(f))
            check_u8("rgb %s[%d]" % (tag, i), got, f["rgb_" + tag][i], RGB_ULPS * U)


def test_fixture_is_what_the_issue_asks_for():
    f = load()
    assert os.path.getsize(os.path.join(GOLD, "g13_video_types.npz")) < os.path.getsize(os.path.join(GOLD, "g67_backprojection.npz"))
    for tag, (persp, n, size) in SETS.items():
        assert f["rast_" + tag].shape == (n, size, size, 4) and f["c2ws_" + tag].shape == (n, 4, 4)
        cov = f["alpha_" + tag] > 0
        assert np.array_equal(cov, f["rast_" + tag][..., 3] > 0) and cov[0].any() and not cov[0].all()
    # a later perspective frame reaches depths on both sides of frame 0's (lo, hi): 'first frame only' shows
    for t in NORMALIZE:
        lo, hi = f["scale_%s_p" % t]
        later = f["raw_%s_p" % t][1:][f["alpha_p"][1:] > 0]
        assert later.min() < lo and later.max() > hi
        x = f["%s_p" % t][1:][f["alpha_p"][1:] > 0]
        assert x.min() < 0.0 and x.max() > 1.0


@pytest.mark.parametrize("video_type", GEOM_TYPES)
def test_numpy_restatement_reproduces_reference_frames(video_type):
    """from the fixture's rast and the per-vertex attributes the reference interpolated: bit-exact position / depth arms, the derived
    bounds of the module docstring for the norm arms"""
    f = load()
    for tag, (persp, n, size) in SETS.items():
        ref, alpha = fixture_frames(f, video_type, tag), f["alpha_" + tag]
        scale = None
        if video_type in NORMALIZE:
            scale = value_range(video_type, f["rast_" + tag][0], f["faces"], fixture_attr(f, video_type, tag, 0))
            print("%s %s (lo, hi): restated %r, reference %r" % (video_type, tag, scale, tuple(f["scale_%s_%s" % (video_type, tag)])))
            if video_type == "z_depth":
                assert np.array_equal(np.asarray(scale, F32), f["scale_%s_%s" % (video_type, tag)])
            else:       # two norms, each within 2.5u of the exact value
                assert np.all(np.abs(np.asarray(scale, np.float64) - f["scale_%s_%s" % (video_type, tag)]) <= 5 * U * scale[1])
            scale = f["scale_%s_%s" % (video_type, tag)]
        for i in range(n):
            rgba, u8 = shade(video_type, f["rast_" + tag][i], f["faces"], fixture_attr(f, video_type, tag, i), scale2=scale,
                             ndc=video_type not in NORMALIZE)
            check_frame("%s %s[%d]" % (video_type, tag, i), rgba, u8, ref[i], alpha[i], float_bound(f, video_type, tag))


@pytest.mark.parametrize("video_type", ["camera_normal", "camera_position", "z_depth", "distance"])
def test_vertex_attributes_from_mesh_and_cameras(video_type):
    """the per-view vertex attributes in the build's operation order against the reference's torch.matmul ones, and the frames that
    follow from them (what export_orbit_video renders end to end)"""
    f = load()
    smax = float(np.abs(f["verts"]).sum(-1).max() + 2.8 + 1.0)
    for tag, (persp, n, size) in SETS.items():
        ref, alpha = fixture_frames(f, video_type, tag), f["alpha_" + tag]
        attrs = [vertex_attr(video_type, f["verts"], f["v_nrm"], f["c2ws_" + tag][i], f["intr_" + tag], persp) for i in range(n)]
        for i in range(n):
            d = np.abs(attrs[i].astype(np.float64) - fixture_attr(f, video_type, tag, i)).max()
            print("%s %s[%d]: per-vertex max|diff| %.3g" % (video_type, tag, i, d))
            if video_type == "z_depth":      # the w row is -w2c[2] (perspective) or (0, 0, 0, 1): equal here, so the arm stays bit-exact end to end
                assert d == 0.0
            elif video_type == "camera_normal":
                assert d <= CAMNRM_ULPS * U
            else:
                assert d <= 8 * U * smax
        scale = None
        if video_type in NORMALIZE:
            scale = np.asarray(value_range(video_type, f["rast_" + tag][0], f["faces"], attrs[0]), F32)
        for i in range(n):
            rgba, u8 = shade(video_type, f["rast_" + tag][i], f["faces"], attrs[i], scale2=scale, ndc=video_type not in NORMALIZE)
            check_frame("%s %s[%d] own attributes" % (video_type, tag, i), rgba, u8, ref[i], alpha[i],
                        float_bound(f, video_type, tag, own_attrs=True))


def test_first_frame_range_only():
    """normalising every frame with its own (min, max) would keep all values in [0, 1]; the reference's do not"""
    f = load()
    for t in NORMALIZE:
        i = 1
        own = value_range(t, f["rast_p"][i], f["faces"], fixture_attr(f, t, "p", i))
        rgba, _ = shade(t, f["rast_p"][i], f["faces"], fixture_attr(f, t, "p", i), scale2=own)
        assert not np.array_equal(rgba[..., :3], fixture_frames(f, t, "p")[i])
        cov = f["alpha_p"][i] > 0
        assert fixture_frames(f, t, "p")[i][cov].max() > 1.0 and fixture_frames(f, t, "p")[i][cov].min() < 0.0


def test_generator_reproduces_committed_fixture(tmp_path):
    """re-runs tests/golden/make_golden_video_types.py and compares every array bit for bit.  The generator imports the reference's own
    Python, which lives outside this repository (make_golden.REF): the test runs wherever that tree is present (the build machines) and
    skips, before doing any work, where it is not (e.g. a GPU box that holds the repository alone)."""
    sys.path.insert(0, GOLD)
    try:
        from make_golden import REF
    finally:
        sys.path.remove(GOLD)
    if not os.path.isdir(REF):
        pytest.skip("the reference tree is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_video_types.py"), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    new, old = np.load(str(tmp_path / "g13_video_types.npz")), load()
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), k


def test_arguments_are_checked_before_any_gpu_work(tmp_path):
    """ext, then video_type (export_nvdiffrast_video.py:155-166); 'albedo' is on the list but uv_rendering cannot render it: KeyError (:103)"""
    from unitex_amd.texturetools.video import VideoExporter
    ex = VideoExporter.__new__(VideoExporter)       # no device needed up to the argument checks
    ex.device, ex.normal_weighting = "cpu", "angle"
    with pytest.raises(AssertionError):
        ex.export_orbit_video(None, str(tmp_path / "a.avi"), video_type="z_depth")
    with pytest.raises(AssertionError):
        ex.export_orbit_video(None, str(tmp_path / "a.mp4"), video_type="normal")
    with pytest.raises(KeyError):
        ex.export_orbit_video(None, str(tmp_path / "a.mp4"), video_type="albedo")


def test_abi_binds_the_gbuffer_entry_points():
    from unitex_amd import _lib
    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "unitex_hip.h")).read()
    for n in ("utx_gbuffer_shade", "utx_gbuffer_range", "utx_camera_normals"):
        assert n in _lib.SYMBOLS and hasattr(lib, n) and n + "(" in hdr
    from unitex_amd.texturetools import ops
    for t, m in ops.GBUFFER_MODES.items():
        assert "#define UTX_GBUF_%s %d\n" % (t.upper(), m) in hdr
