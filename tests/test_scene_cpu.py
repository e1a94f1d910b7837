"""Environment renderer without a GPU: the fp64 restatement (tests/support/scene_ref.py) against the reference's own torch code (fixture G23,
tests/golden/make_golden_scene.py), the layout functions (pure torch, they run here), the C ABI's argument checks and the Python refusals.

The reference computes in fp32; the restatement is held to the reference's OWN rounding, measured here once and held with a factor 2, since both
sides are deterministic on the CPU:
    rays_d 1.12e-7   uv 7.82e-8 (u on the circle)   the panorama's direction grid 2.38e-7   cubemap_to_latlong 4.88e-7
    bake uv 1.26e-4 relative to max(1, |uv|) over every (view, texel) (the depth comes within 1e-4 of 0), 5.09e-7 inside the views
    baked panorama 3.12e-6 (the uv error times the views' contrast), 4.13e-7 at the reference's own uv"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import pbr_ref as PC
from tests.support import scene_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
H, W, N, HT, WT, M = 8, 12, 4, 6, 12, 5
# the reference's own fp32 rounding against the fp64 restatement, measured (printed below), times 2
_R = S.REF_ROUNDING
TOL_BAKE_UV_INSIDE = 2 * _R["bake_uv_inside"]
TOL_RAYS, TOL_UV, TOL_DIR, TOL_C2L, TOL_BAKE_UV, TOL_LOOKUP, TOL_BAKE = (2 * _R[k] for k in ("rays", "uv", "texel_dir", "cubemap_to_latlong", "bake_uv", "bake_at_own_uv", "bake"))


def test_rays_and_uv_restatement_against_g23():
    f = S.load_g23()
    ro, rd, bound = S.rays(f["c2ws"], f["intrinsics"], H, W)
    assert ro.astype(F32).tobytes() == f["rays_o"].tobytes() == f["inv_rays_o"].tobytes()
    e_rays = np.abs(rd - f["rays_d"]).max()
    e_uv = max(S.circle_diff(S.dir_uv(rd)[..., 0], f["uv"][..., 0]).max(), np.abs(S.dir_uv(rd)[..., 1] - f["uv"][..., 1]).max())
    print("reference rounding: rays_d %.3g, uv %.3g; counted kernel bound on rays_d: at most %.3g" % (e_rays, e_uv, bound.max()))
    assert e_rays <= TOL_RAYS and e_uv <= TOL_UV
    assert np.array_equal(f["rays_d"], f["inv_rays_d"])
    assert np.abs(np.linalg.norm(rd, axis=-1) - 1).max() < 1e-15


@pytest.mark.parametrize("Cc", [3, 4])
def test_lookups_at_the_logged_coordinates(Cc):
    f = S.load_g23()
    cube, lat = f["cubemap%d" % Cc], f["latlong%d" % Cc]
    # what the reference handed to dr.texture is what it returned as rays_d / uv, and its outputs are the lookups there
    assert np.array_equal(f["render%d_cube_coord" % Cc], f["rays_d"]) and np.array_equal(f["render%d_latlong_coord" % Cc], f["uv"])
    assert np.array_equal(f["cubemap_attr%d" % Cc], f["render%d_cube_lookup" % Cc]) and np.array_equal(f["latlong_map_attr%d" % Cc], f["render%d_latlong_lookup" % Cc])
    assert np.array_equal(PC.cube_lookup(cube, f["rays_d"]).astype(F32), f["cubemap_attr%d" % Cc])
    assert np.array_equal(S.wrap_linear(lat, f["uv"]).astype(F32), f["latlong_map_attr%d" % Cc])
    # cubemap_to_latlong: the reference's fp32 direction grid against the restatement's (fp64, rounded once), then the same cube rule
    coord = f["c2l%d_cube_coord" % Cc][0]
    e_dir = np.abs(coord - S.texel_dirs(HT, WT)).max()
    print("reference rounding: the panorama's direction grid %.3g" % e_dir)
    assert e_dir <= TOL_DIR, e_dir
    assert np.array_equal(PC.cube_lookup(cube, coord).astype(F32), f["cubemap_to_latlong%d" % Cc])
    K = 2 * 2 * np.sqrt(3.0) * (N / 2) * (cube.max() - cube.min())
    e_c2l = np.abs(S.cubemap_to_latlong(cube, HT, WT) - f["cubemap_to_latlong%d" % Cc]).max()
    print("reference rounding: cubemap_to_latlong %.3g (its direction error times the texel contrast allows %.3g)" % (e_c2l, K * e_dir))
    assert e_c2l <= TOL_C2L <= K * e_dir


@pytest.mark.parametrize("Cc", [3, 4])
def test_bake_restatement_against_g23(Cc):
    f = S.load_g23()
    uv, depth, alpha, bound, dbound = S.bake_project(f["w2cs"], f["projections"], HT, WT)
    assert S.bake_margin_ok(uv, depth, bound, dbound)
    assert (np.abs(np.abs(uv) - 1) >= 1e-4).all() and (np.abs(depth) >= 1e-4).all(), "the generator's margin"
    assert np.array_equal(alpha[..., None].astype(F32), f["inv_uv_alpha"]), "masks: exact, every (view, texel)"
    assert abs(alpha.mean() - 0.111) < 0.001 and abs((alpha.sum(0) > 0).mean() - 0.444) < 0.001
    e_uv = (np.abs(uv - f["inv_uv"]) / np.maximum(1.0, np.abs(uv))).max()
    img = f["images%d" % Cc]
    want, cnt = S.bake(img, uv, alpha)
    e_bake = np.abs(want - f["inv_latlong_map_attr%d" % Cc]).max()
    print("reference rounding: bake uv %.3g (relative), panorama %.3g; counted kernel bounds: uv %.3g, panorama %.3g" %
          (e_uv, e_bake, (bound / np.maximum(1.0, np.abs(uv))).max(), S.bake_bound(img, cnt).max()))
    assert e_uv <= TOL_BAKE_UV and e_bake <= TOL_BAKE
    unseen = cnt == 0
    assert unseen.any() and (~unseen).any() and (f["inv_latlong_map_attr%d" % Cc][unseen] == 0).all() and (want[unseen] == 0).all()
    assert (want == 1).any(), "the clamp shows"
    # at the reference's own uv only the sum and the blend remain
    at_ref, _ = S.bake(img, f["inv_uv"], f["inv_uv_alpha"])
    e_at = np.abs(at_ref - f["inv_latlong_map_attr%d" % Cc]).max()
    e_in = np.abs(uv - f["inv_uv"])[alpha].max()
    print("reference rounding: panorama at its own uv %.3g, uv inside the views %.3g" % (e_at, e_in))
    assert e_at <= TOL_LOOKUP and e_in <= TOL_BAKE_UV_INSIDE


def test_layouts_and_pcd_against_g23():
    from unitex_amd.texturetools import renderer_scene as RS
    f = S.load_g23()
    cube = torch.from_numpy(f["cubemap3"])
    flat = RS.cubemap_to_flatten(cube)
    assert np.array_equal(flat.numpy(), f["flatten"]) and flat.shape == (3 * N, 4 * N, 3)
    assert torch.equal(RS.flatten_to_cubemap(flat), cube), "the round trip is the identity"
    kjl = RS.cubemap_to_flatten_kjl(cube)
    assert np.array_equal(kjl.numpy(), f["flatten_kjl"])
    assert np.array_equal(RS.flatten_to_cubemap(kjl).numpy(), f["flatten_kjl_cubemap"])
    g = torch.linspace(-0.75, 0.75, N)
    assert np.array_equal(RS.grid_to_cube(g[None, :], g[:, None]).numpy(), f["grid_to_cube"])
    for s in range(6):      # the same face order and orientation as the cube rule's
        assert np.array_equal(f["grid_to_cube"][s].astype(np.float64), PC.cube_to_dir(s, *np.meshgrid(g.numpy().astype(np.float64), g.numpy().astype(np.float64))))
    pcd = RS.latlong_depth_to_pcd(torch.from_numpy(f["pcd_depth"])).numpy()
    assert np.abs(pcd - f["pcd"]).max() <= 4 * S.U * f["pcd_depth"].max()
    assert np.abs(f["pcd"] - f["pcd_depth"] * S.texel_dirs(HT, WT)).max() <= 4 * S.U * f["pcd_depth"].max()


def test_recorded_quirks():
    f = S.load_g23()
    assert list(f["keys_latlong_without_uv"]) == ["rays_d", "rays_o"], "render_latlong_map without render_uv returns no map in the reference"
    assert list(f["keys_all_flags"]) == ["cubemap_attr", "latlong_map_attr", "rays_d", "rays_o", "uv"]
    assert int(f["inverse_batched_intrinsics_fail"]) == 1
    # cubemap_to_latlong and latlong_to_cubemap are not inverses of each other
    lat = S.cubemap_to_latlong(f["cubemap3"], HT, WT)
    back, _ = PC.latlong_to_cubemap(lat, N)
    assert np.abs(back - f["cubemap3"]).max() > 0.05


def test_abi_binds_the_entry_points_and_checks_arguments():
    from unitex_amd import _lib
    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "unitex_hip.h")).read()
    for name, nargs in (("utx_scene_render", 18), ("utx_cubemap_to_latlong", 8), ("utx_scene_bake_latlong", 14)):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and ("int %s(" % name) in hdr
        assert len(_lib.SYMBOLS[name][1]) == nargs, name
    # the argument checks come before any device call, so they run here: no context, made-up addresses that are never read
    p = C.c_void_p(4096)
    ok = lambda **k: [k.get("c2ws", p), k.get("intr", p), k.get("stride", 0), k.get("B", 2), k.get("H", 4), k.get("W", 4), k.get("cube", p), k.get("N", 4),
                      k.get("lat", p), k.get("Hi", 4), k.get("Wi", 8), k.get("C", 3), k.get("rays", p), k.get("cattr", p), k.get("uv", p), k.get("lattr", p), None]
    for bad in (dict(c2ws=None), dict(intr=None), dict(stride=3), dict(B=0), dict(H=0), dict(W=-1), dict(cube=None), dict(N=0), dict(N=3), dict(N=8194),
                dict(lat=None), dict(Hi=0), dict(Wi=0), dict(C=0), dict(C=5), dict(rays=None, cattr=None, uv=None, lattr=None)):
        assert lib.utx_scene_render(None, *ok(**bad)) == -2, bad
    assert lib.utx_cubemap_to_latlong(None, None, 4, 3, 4, 8, p, None) == -2 and lib.utx_cubemap_to_latlong(None, p, 4, 3, 4, 8, None, None) == -2
    for N_, C_, Ht, Wt in ((0, 3, 4, 8), (3, 3, 4, 8), (8194, 3, 4, 8), (4, 0, 4, 8), (4, 5, 4, 8), (4, 3, 0, 8), (4, 3, 4, 0)):
        assert lib.utx_cubemap_to_latlong(None, p, N_, C_, Ht, Wt, p, None) == -2, (N_, C_, Ht, Wt)
    okb = lambda **k: [k.get("w2c", p), k.get("proj", p), k.get("img", p), k.get("M", 2), k.get("H", 4), k.get("W", 4), k.get("C", 3), k.get("Ht", 4),
                       k.get("Wt", 8), k.get("uv", p), k.get("alpha", p), k.get("out", p), None]
    for bad in (dict(w2c=None), dict(proj=None), dict(img=None), dict(M=0), dict(H=0), dict(W=0), dict(C=0), dict(C=5), dict(Ht=0), dict(Wt=0),
                dict(uv=None, alpha=None, out=None)):
        assert lib.utx_scene_bake_latlong(None, *okb(**bad)) == -2, bad


def test_python_refusals_need_no_gpu(monkeypatch):
    from unitex_amd.texturetools import ops
    from unitex_amd.texturetools.renderer_scene import NVDiffRendererScene

    def no_ctx(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "get_ctx", no_ctx)
    f = S.load_g23()
    c2ws, intr, img = torch.from_numpy(f["c2ws"]), torch.from_numpy(f["intrinsics"]), torch.from_numpy(f["images3"])
    r = NVDiffRendererScene(device="cpu")
    assert r.latlong_map is None and r.cubemap is None
    r.enable_nvdiffrast_cuda_ctx(), r.enable_nvdiffrast_opengl_ctx()
    with pytest.raises(ValueError, match="cubemap"):
        r.perspective_rendering(c2ws, intr, (H, W), render_cubemap=True)
    with pytest.raises(ValueError, match="lat-long"):
        r.perspective_rendering(c2ws, intr, (H, W), render_uv=True, render_latlong_map=True)
    with pytest.raises(NotImplementedError):
        r.perspective_inverse_rendering_torch(c2ws, intr, img, (H, W), (HT, WT), render_cubemap=True)
    with pytest.raises(NotImplementedError, match="scipy"):
        r.perspective_inverse_rendering_scipy(c2ws, intr, img, (H, W), (HT, WT))
    with pytest.raises(TypeError):
        r.perspective_rendering(c2ws, intr, (H, W), render_depth=True)
    with pytest.raises(TypeError):
        r.perspective_inverse_rendering_torch(c2ws, intr, img, (H, W), (HT, WT), antialias=True)
    with pytest.raises(ValueError, match="intrinsics"):
        r.perspective_rendering(c2ws, intr[None].expand(2, 3, 3), (H, W))
    with pytest.raises(ValueError, match="images"):
        r.perspective_inverse_rendering_torch(c2ws, intr, None, (H, W), (HT, WT), render_uv=True, render_latlong_map=True)
    r2 = NVDiffRendererScene(device="cpu", latlong_map=torch.from_numpy(f["latlong3"]), cubemap=torch.from_numpy(f["cubemap3"]))
    r2.clear()
    assert r2.latlong_map is None and r2.cubemap is None


def test_from_images_and_the_kjl_layout():
    from PIL import Image
    from unitex_amd.texturetools import renderer_scene as RS
    rng = np.random.default_rng(3)
    faces = [Image.fromarray(rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)) for _ in range(6)]
    pano = Image.fromarray(rng.integers(0, 256, (4, 8), dtype=np.uint8))      # grey: repeated to RGB
    r = RS.NVDiffRendererScene.from_images(device="cpu", latlong_map=pano, cubemaps=faces)
    want = np.stack([np.asarray(im, F32) / F32(255) for im in faces])
    assert np.array_equal(r.cubemap.numpy(), want) and r.latlong_map.shape == (4, 8, 3) and torch.equal(r.latlong_map[..., 0], r.latlong_map[..., 2])
    k = RS.NVDiffRendererScene.from_images(device="cpu", cubemaps=faces, cubemap_kjl=True)
    assert k.latlong_map is None and torch.equal(k.cubemap, RS.flatten_to_cubemap(RS.cubemap_to_flatten_kjl(torch.from_numpy(want))))
    assert r.update_from_images(cubemaps=faces, cubemap_kjl=True) is r and r.latlong_map is None and torch.equal(r.cubemap, k.cubemap)
