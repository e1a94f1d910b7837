"""Screen-space buffers (NVDiffRendererInverse.simple_rendering / utx_screen_gbuffer), CPU side: the table of the reference's simple_rendering
(render/nvdiffrast/renderer_base.py:101-350) restated in numpy, in the kernel's operation order, against the reference's own buffers (fixture
G18, tests/golden/make_golden_simple_rendering.py; alpha = coverage, dr.antialias stubbed).  The restatement (the screen form of table), the map
lookups (oracle/pixel_ref.py) and the bounds with their derivation (MAP_BOUND for 'bilinear', bit-exact elsewhere) are in oracle/gbuffer_ref.py;
the GPU module (tests/test_simple_rendering_gpu.py) uses them too."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.gbuffer_ref import ATLAS, CHANNELS, FILL, GEOMETRY, MODES, SCREEN, SETS, UNBUILT, VIEWS, F32, F64, background_cases, bounds, check, map_bound, table, v_uv
from oracle.gbuffer_ref import load_g18 as load
from oracle.pixel_ref import grid_unnormalize

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(H, W), B = SCREEN, VIEWS


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
        ix, iy = grid_unnormalize(uv[..., 0], Wt), grid_unnormalize(uv[..., 1], Ht)
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
    got = table(rast, faces, f["verts"], f["v_nrm"], f["v_pos_cam_" + tag], f["v_nrm_cam_" + tag], f["clip_w_" + tag], v_uv(f))
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
