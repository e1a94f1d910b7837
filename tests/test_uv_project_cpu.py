"""Atlas-space view projection and face / vertex visibility, CPU side: the numpy restatement (oracle/uv_project_ref.py) of utx_visible_faces_rays,
utx_visible_faces_raster, utx_erode_faces, utx_visible_vertices and utx_uv_project against the reference's own results (fixture G19,
tests/golden/make_golden_uv_project.py), the argument handling of NVDiffRendererInverse and the C entry points' argument checks.

Bounds (u = 2^-24; none of them was taken from the code under test):
  * the masks are sets of integers: EXACT.  The ray caster of the fixture is a float64 brute force and every ray of the fixture passes the margin of
    oracle/uv_project_ref.py (asserted when the fixture is made and again here), so a float32 traversal has to find the same faces.
  * uv_alpha, uv: a select and utx_interpolate's one expression on the fixture's own v_ndc: BIT-EXACT.
  * map_attr in 'nearest' and 'nvdiffrast', every background form: BIT-EXACT (one tap; the restated lookup of G67n).
  * map_attr in 'bilinear': torch's CPU grid_sample in the fixture, which is not one fixed sequence of roundings.  The counted bound of
    oracle/gbuffer_ref.py, MAP_BOUND = (14 M + 4 (Wm + Hm) R) u, is a function of the map's size and range and is evaluated for the
    maps of this fixture by that module's map_bound(): 174 u for the 16 x 24 maps and 78 u for the 8 x 8 ones at M = R = 1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import uv_project_ref as R
from oracle.pixel_ref import grid_unnormalize
from oracle.uv_project_ref import ATLAS, B, MODES, RASTER_SIZE, SETS, cases, check_map, load

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, U = np.float32, np.float64, 2.0 ** -24


def test_fixture_is_what_the_issue_asks_for():
    f = load()
    Fn, V = f["faces"].shape[0], f["verts"].shape[0]
    assert f["rast2d"].shape == ATLAS + (4,) and f["faces"].dtype == np.int32
    assert f["map_0"].shape == (B, 16, 24, 3) and f["map_1"].shape == (B, 8, 8, 5)
    plate = np.arange(Fn) >= Fn - 2
    for tag, perspective in SETS:
        assert f["c2ws_" + tag].shape == (B, 4, 4) and f["v_ndc_" + tag].shape == (B, V, 2)
        assert f["uv_" + tag].shape == (B,) + ATLAS + (2,) and f["uv_alpha_" + tag].shape == (B,) + ATLAS + (1,)
        assert f["rast_map_0_" + tag].shape == (B, 16, 24, 4) and f["rast_map_1_" + tag].shape == (B, 8, 8, 4)
        mask, hit, ok = R.visible_faces_rays(f["verts"], f["faces"], f["c2ws_" + tag], perspective)
        assert ok.all(), "a ray of the fixture fails the margin"
        aimed = np.arange(Fn)[None]
        other = (hit != aimed) & (hit >= 0)
        assert other.any(1).all()                                                                    # a ray marks another face, in every view
        assert (other & plate[np.clip(hit, 0, None)] & ~plate[None]).any(1).all()                    # hidden by the plate, in every view
        assert (other & ~plate[np.clip(hit, 0, None)] & ~plate[None]).any(1).all()                   # hidden by the cylinder itself, in every view
        vis = f["uv_alpha_" + tag][..., 0] > 0
        for Hm, Wm in ((16, 24), (8, 8)):      # G18's outside-tap condition, per filter and map, on the texels the views see
            ix, iy = grid_unnormalize(f["uv_" + tag][..., 0], Wm), grid_unnormalize(f["uv_" + tag][..., 1], Hm)
            assert (vis & ((np.floor(ix) < 0) | (np.floor(ix) + 1 >= Wm) | (np.floor(iy) < 0) | (np.floor(iy) + 1 >= Hm))).any()         # bilinear
            assert (vis & ((np.rint(ix) < 0) | (np.rint(ix) >= Wm) | (np.rint(iy) < 0) | (np.rint(iy) >= Hm))).any()                     # nearest
            su = f["uv_" + tag] * F32(0.5) + F32(0.5)
            su = (su - np.floor(su)) * np.array([Wm, Hm], F32) - F32(0.5)
            assert (vis & ((np.floor(su) < 0) | (np.floor(su) + 1 >= np.array([Wm, Hm]))).any(-1)).any()                                 # nvdiffrast wraps
        assert any((vis & (f["uv_alpha_map_%d_%s" % (i, tag)][..., 0] < 1)).any() for i in (0, 1))   # vis true but cov < 1
    # what the reference does with the calls this build refuses or widens
    assert str(f["refusal_uv_with_camera_flags"]) == "TypeError" and str(f["refusal_uv_without_cameras"]) == "AttributeError"
    assert str(f["refusal_map_attr_without_uv"]) == "alpha,mask"      # dropped without a word: no 'map_attr' in the result


@pytest.mark.parametrize("tag,perspective", SETS)
def test_visibility_restatement_reproduces_the_fixture(tag, perspective):
    f = load()
    Fn, V = f["faces"].shape[0], f["verts"].shape[0]
    rays = R.visible_faces_rays(f["verts"], f["faces"], f["c2ws_" + tag], perspective)[0]
    assert np.array_equal(rays, f["faces_rays_e0_" + tag] > 0)
    assert np.array_equal(R.erode_faces(rays, f["faces"], V, 1), f["faces_rays_e1_" + tag] > 0)
    assert np.array_equal(R.erode_faces(rays, f["faces"], V, 0), rays)
    assert np.array_equal(R.visible_vertices(rays, f["faces"], V), f["verts_rays_e0_" + tag] > 0)
    rast = R.visible_faces_raster(f["rast_view_" + tag], Fn)
    assert np.array_equal(rast, f["faces_raster_e0_" + tag] > 0)
    assert np.array_equal(R.erode_faces(rast, f["faces"], V, 1), f["faces_raster_e1_" + tag] > 0)
    for e in (0, 1):
        assert np.array_equal(R.visible_vertices(f["faces_raster_e%d_%s" % (e, tag)], f["faces"], V), f["verts_raster_e%d_%s" % (e, tag)] > 0)
    two = R.erode_faces(rays, f["faces"], V, 2)
    assert np.array_equal(two, R.erode_faces(R.erode_faces(rays, f["faces"], V, 1), f["faces"], V, 1)) and two.sum() < (f["faces_rays_e1_" + tag] > 0).sum()


@pytest.mark.parametrize("tag,perspective", SETS)
def test_projection_restatement_reproduces_the_fixture(tag, perspective):
    f = load()
    mask = f["faces_rays_e0_" + tag]
    got = R.uv_project(f["rast2d"], f["faces"], mask, f["v_ndc_" + tag])
    assert got["uv"].tobytes() == f["uv_" + tag].tobytes() and got["uv_alpha"].tobytes() == f["uv_alpha_" + tag].tobytes()
    worst = 0.0
    for key, m, i, mode, bg in cases(f, tag):
        got = R.uv_project(f["rast2d"], f["faces"], mask, f["v_ndc_" + tag], m, f["rast_map_%d_%s" % (i, tag)], mode, bg)
        assert got["uv"].tobytes() == f["uv_" + tag].tobytes()      # uv is not gated by cov
        assert got["uv_alpha"].tobytes() == f["uv_alpha_map_%d_%s" % (i, tag)].tobytes(), key
        dev = check_map(key, got["map_attr"], f[key], mode, m)
        worst = max(worst, dev if mode == "bilinear" else 0.0)
    print("bilinear map_attr of the restatement against G19, set %s: at most %.2f u" % (tag, worst))


def test_abi_binds_the_entry_points_and_checks_arguments():
    from unitex_amd import _lib
    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "unitex_hip.h")).read()
    for name, nargs in (("utx_visible_faces_rays", 12), ("utx_visible_faces_raster", 8), ("utx_erode_faces", 9), ("utx_visible_vertices", 8),
                        ("utx_uv_project", 24)):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and ("int %s(" % name) in hdr
        assert len(_lib.SYMBOLS[name][1]) == nargs, name
    assert "#define UTX_VF_STACK_WALK 1\n" in hdr and "#define UTX_VF_FACE_ORDER 2\n" in hdr
    # the argument checks come before any device call, so they run here: no context, made-up addresses that are never read
    p, q = C.c_void_p(4096), C.c_void_p(4096 + 8)
    assert lib.utx_visible_faces_rays(None, None, p, p, 4, p, 1, 1, 0, p, None, None) == -2          # no tree
    assert lib.utx_visible_faces_rays(None, p, p, p, 0, p, 1, 1, 0, p, None, None) == -2             # F <= 0
    assert lib.utx_visible_faces_rays(None, p, p, p, 4, p, 0, 1, 0, p, None, None) == -2             # B <= 0
    assert lib.utx_visible_faces_rays(None, p, p, p, 4, p, 1, 1, 4, p, None, None) == -2             # unknown flag
    assert lib.utx_visible_faces_rays(None, p, p, p, 4, p, 1, 1, 0, None, None, None) == -2          # no mask
    assert lib.utx_visible_faces_raster(None, None, 1, 4, 4, 4, p, None) == -2 and lib.utx_visible_faces_raster(None, p, 1, 4, 4, 0, p, None) == -2
    assert lib.utx_erode_faces(None, None, p, 1, 4, 4, 1, p, None) == -2 and lib.utx_erode_faces(None, p, p, 1, 4, 0, 1, p, None) == -2
    assert lib.utx_erode_faces(None, p, p, 1, 4, 4, 1, None, None) == -2                             # no scratch for depth > 0
    assert lib.utx_visible_vertices(None, p, p, 1, 4, 4, None, None) == -2 and lib.utx_visible_vertices(None, p, p, 1, 0, 4, p, None) == -2
    ok = lambda **k: [k.get("rast2d", p), p, k.get("F", 4), k.get("mask", p), p, k.get("V", 4), k.get("B", 3), 4, 4, k.get("map", p), k.get("Bm", 1), 4, 4,
                      k.get("C", 3), k.get("rast_map", p), k.get("filter", 0), k.get("bg_kind", 0), 0.0, k.get("bg", None), k.get("uv", p), p, k.get("out", p), None]
    for bad in (dict(rast2d=None), dict(rast2d=q), dict(mask=None), dict(uv=None), dict(F=0), dict(V=0), dict(B=0), dict(Bm=2), dict(C=0), dict(rast_map=None),
                dict(out=None), dict(filter=3), dict(bg_kind=4), dict(bg_kind=2), dict(bg_kind=3)):
        assert lib.utx_uv_project(None, *ok(**bad)) == -2, bad


def test_python_argument_checks_need_no_gpu(monkeypatch):
    """every refusal of simple_inverse_rendering and of the two visibility methods comes before the library is touched"""
    import torch
    from unitex_amd.texturetools import ops
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse

    def no_ctx(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "get_ctx", no_ctx)
    inv = NVDiffRendererInverse(device="cpu")
    f = load()
    c2ws, intr = torch.from_numpy(f["c2ws_p"].copy()), torch.from_numpy(f["intr_p"].copy())
    sir = inv.simple_inverse_rendering
    with pytest.raises(NotImplementedError, match="render_uv"):
        sir(None, ATLAS, render_uv=True)
    with pytest.raises(NotImplementedError, match="render_uv"):
        sir(None, ATLAS, render_uv=True, intrinsics=intr)
    with pytest.raises(NotImplementedError, match="render_map_attr"):
        sir(c2ws, ATLAS, render_map_attr=True, map_attr=torch.zeros(4, 4, 3))
    with pytest.raises(ValueError, match="intrinsics"):
        sir(c2ws, ATLAS, render_uv=True)
    with pytest.raises(ValueError, match="intrinsics"):
        sir(c2ws, ATLAS, render_uv=True, intrinsics=None)
    with pytest.raises(TypeError, match="intrinsics"):
        sir(c2ws, ATLAS, intrinsics=intr, render_world_normal=True)
    with pytest.raises(ValueError, match="map_attr"):
        sir(c2ws, ATLAS, render_uv=True, render_map_attr=True, intrinsics=intr)
    for bad in (torch.zeros(4, 3), torch.zeros(1, 1, 4, 4, 3), torch.zeros(2, 4, 4, 3), torch.zeros(4, 4, 4, 3), torch.zeros(4, 0, 3)):
        with pytest.raises(ValueError, match="map_attr"):
            sir(c2ws, ATLAS, render_uv=True, render_map_attr=True, intrinsics=intr, map_attr=bad)
    with pytest.raises(ValueError, match="grid_interpolate_mode"):
        sir(c2ws, ATLAS, render_uv=True, intrinsics=intr, grid_interpolate_mode="bicubic")
    with pytest.raises(ValueError, match="visible_faces"):
        sir(c2ws, ATLAS, render_uv=True, intrinsics=intr, visible_faces="optix")
    with pytest.raises(ValueError, match="raster"):
        sir(c2ws, ATLAS, render_uv=True, intrinsics=intr, visible_faces="raster")      # the raster method takes its size from map_attr
    for flag in ("render_voxel_attr", "render_all_point_cloud", "render_visible_point_cloud"):
        with pytest.raises(NotImplementedError, match=flag):
            sir(c2ws, ATLAS, render_uv=True, intrinsics=intr, **{flag: True})
    with pytest.raises(TypeError, match="render_albedo"):
        sir(c2ws, ATLAS, render_uv=True, intrinsics=intr, render_albedo=True)
    for method in (inv.get_visible_faces, inv.get_visible_vertices):
        with pytest.raises(ValueError, match="raster"):
            method(c2ws, method="raster")
        with pytest.raises(ValueError, match="raster"):
            method(c2ws, method="raster", intrinsics=intr)
        with pytest.raises(ValueError, match="raster"):
            method(c2ws, method="raster", render_size=32)
        with pytest.raises(ValueError, match="method"):
            method(c2ws, method="embree")
        with pytest.raises(ValueError, match="erode_neighbor"):
            method(c2ws, erode_neighbor=-1)
        with pytest.raises(ValueError, match="c2ws"):
            method(c2ws[0])
    x = torch.zeros(4, 4, 4)
    with pytest.raises(ValueError, match="filter"):
        ops.uv_project(x, torch.zeros(2, 3, dtype=torch.int32), x, x, filter="cubic")
    with pytest.raises(ValueError, match="face_mask"):
        ops.uv_project(x, torch.zeros(2, 3, dtype=torch.int32), torch.zeros(3, 5, dtype=torch.uint8), torch.zeros(3, 7, 2))
    with pytest.raises(ValueError, match="v_ndc"):
        ops.uv_project(x, torch.zeros(2, 3, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.uint8), torch.zeros(2, 7, 2))
    with pytest.raises(ValueError, match="map_attr"):
        ops.uv_project(x, torch.zeros(2, 3, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.uint8), torch.zeros(3, 7, 2), torch.zeros(2, 4, 4, 3), x)
    with pytest.raises(ValueError, match="rast_map"):
        ops.uv_project(x, torch.zeros(2, 3, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.uint8), torch.zeros(3, 7, 2), torch.zeros(1, 4, 4, 3), None)


def test_generator_reproduces_committed_fixture(tmp_path):
    """re-runs tests/golden/make_golden_uv_project.py and compares every array bit for bit.  The generator imports the reference's own Python, which
    lives outside this repository (make_golden.REF): the test runs wherever that tree is present and skips, before doing any work, where it is not."""
    sys.path.insert(0, GOLD)
    try:
        from make_golden import REF
    finally:
        sys.path.remove(GOLD)
    if not os.path.isdir(os.path.join(REF, "TextureTools")):
        pytest.skip("the reference tree is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_uv_project.py"), str(tmp_path)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    f = load()
    with np.load(os.path.join(str(tmp_path), "g19_uv_project.npz"), allow_pickle=False) as g:
        assert sorted(g.files) == sorted(f)
        for k in g.files:
            assert g[k].dtype == f[k].dtype and g[k].shape == f[k].shape and g[k].tobytes() == f[k].tobytes(), k
