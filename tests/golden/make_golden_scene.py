#!/usr/bin/env python
"""Generate the environment-renderer fixture under tests/golden/ from the REFERENCE's own Python, through the same seams as make_golden.py (imported from
there, unchanged):

    python tests/golden/make_golden_scene.py            # writes tests/golden/g23_scene.npz

  G23   TextureTools/texturetools/render/nvdiffrast/renderer_scene.py run on the CPU: NVDiffRendererScene.perspective_rendering with every flag,
        cubemap_to_latlong, perspective_inverse_rendering_torch (render_uv + render_latlong_map), the flatten layouts and latlong_depth_to_pcd.
        c2ws_to_ray_matrices, the inverse renderer and the layouts are pure torch: the fixture pins them as they are.  dr.texture is STUBBED, exactly as in
        G15: boundary_mode='cube' by the fp64 cube rule of oracle/pbr_ref.py:cube_lookup (the library's own, include/unitex_hip.h), every other call by a fp64
        linear lookup with wrap addressing in both axes; coordinates and results are logged.  The fixture therefore pins the reference's arithmetic AROUND
        the lookups, not nvdiffrast's samplers.
        Contents: five orbit cameras (generate_orbit_views_c2ws(5, radius=0.3, height=0.1, theta_0=10 degrees)) with 60 degree intrinsics, views of 8 x 12,
        a cubemap of N = 4, panoramas of 6 x 12, C = 3 and 4, view images with values in [-0.2, 1.5] so that the clamp shows.
        Margin: no texel's uv within 1e-4 of +-1, no depth within 1e-4 of 0, for every (view, texel); the cameras' radius is nudged in steps of 0.003 until that
        holds, so the masks can be demanded bit-exact with no case left out.  Both branches of sum / count must occur (asserted).
        Recorded quirks: the keys returned for render_latlong_map without render_uv; that [M, 3, 3] intrinsics fail in the inverse renderer."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import REF, install_stubs  # noqa: E402

F32 = np.float32
MARGIN = 1e-4
H, W, N, HT, WT, M = 8, 12, 4, 6, 12, 5


def _wrap_linear(tex, uv):
    tex, uv = np.asarray(tex, np.float64), np.asarray(uv, np.float64)
    Hi, Wi = tex.shape[:2]
    x, y = uv[..., 0] * Wi - 0.5, uv[..., 1] * Hi - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    ix = lambda t: np.mod(t.astype(np.int64), Wi)
    iy = lambda t: np.mod(t.astype(np.int64), Hi)
    top = tex[iy(y0), ix(x0)] * (1 - fx) + tex[iy(y0), ix(x0 + 1)] * fx
    bot = tex[iy(y0 + 1), ix(x0)] * (1 - fx) + tex[iy(y0 + 1), ix(x0 + 1)] * fx
    return top * (1 - fy) + bot * fy


def g23(out):
    from oracle import pbr_ref as PC
    R = importlib.import_module("TextureTools.texturetools.render.nvdiffrast.renderer_scene")
    G = importlib.import_module("TextureTools.texturetools.camera.generator")
    CV = importlib.import_module("TextureTools.texturetools.camera.conversion")
    dr = importlib.import_module("nvdiffrast.torch")
    log = {}
    tag = [""]

    def texture(tex, uv, filter_mode="linear", boundary_mode="wrap", **kw):
        assert filter_mode == "linear"
        t, c = tex[0].numpy(), uv.numpy()
        if boundary_mode == "cube":
            r, key = PC.cube_lookup(t, c), "cube"
        else:
            assert boundary_mode == "wrap"
            r, key = _wrap_linear(t, c), "latlong"
        log[tag[0] + key + "_coord"], log[tag[0] + key + "_lookup"] = c.astype(F32), r.astype(F32)
        return torch.from_numpy(r.astype(F32))
    dr.texture = texture

    rng = np.random.default_rng(23)
    intr = G.generate_intrinsics(60.0, 60.0, fov=True, degree=True).to(torch.float32)
    scene = R.NVDiffRendererScene(device="cpu")
    images = {C: torch.from_numpy(rng.uniform(-0.2, 1.5, (M, H, W, C)).astype(F32)) for C in (3, 4)}
    radius = 0.3
    for _ in range(200):      # nudge the cameras until every (view, texel) decides its mask with the margin
        c2ws = G.generate_orbit_views_c2ws(M, radius=radius, height=0.1, theta_0=10.0, degree=True).to(torch.float32)
        inv = scene.perspective_inverse_rendering_torch(c2ws, intr, images[3], (H, W), (HT, WT), render_uv=True, render_latlong_map=True)
        uv, alpha = inv["uv"].numpy().astype(np.float64), inv["uv_alpha"].numpy()
        w2cs = torch.linalg.inv(c2ws)
        projs = CV.intr_to_proj(intr, perspective=True)
        p = np.concatenate([_dirs64(), np.ones((HT, WT, 1))], -1)
        depth = -np.einsum("mij,hwj->mhwi", w2cs.numpy().astype(np.float64), p)[..., 2]
        if (np.abs(np.abs(uv[np.isfinite(uv)]) - 1.0) >= MARGIN).all() and (np.abs(depth) >= MARGIN).all():
            break
        radius += 0.003
    else:
        raise AssertionError("no camera radius gives every texel the margin")
    assert (np.abs(np.abs(uv) - 1.0) >= MARGIN).all() and (np.abs(depth) >= MARGIN).all()
    seen = alpha[..., 0].sum(0) > 0
    assert 0.2 < seen.mean() < 0.8 and 0.05 < alpha.mean() < 0.5, (seen.mean(), alpha.mean())      # both branches of sum / count
    fix = dict(c2ws=c2ws.numpy(), intrinsics=intr.numpy(), radius=np.float64(radius), w2cs=w2cs.numpy(), projections=projs.numpy(),
               inv_rays_o=inv["rays_o"].numpy().copy(), inv_rays_d=inv["rays_d"].numpy(), inv_uv=inv["uv"].numpy(), inv_uv_alpha=alpha,
               seen_fraction=np.float64(seen.mean()), inside_fraction=np.float64(alpha.mean()))
    for C in (3, 4):
        cube = torch.from_numpy(rng.uniform(0.0, 1.0, (6, N, N, C)).astype(F32))
        lat = torch.from_numpy(rng.uniform(0.0, 1.0, (HT, WT, C)).astype(F32))
        scene.cubemap, scene.latlong_map = cube, lat
        tag[0] = "render%d_" % C
        r = scene.perspective_rendering(c2ws, intr, (H, W), render_cubemap=True, render_uv=True, render_latlong_map=True)
        if C == 3:
            fix.update(rays_o=r["rays_o"].numpy().copy(), rays_d=r["rays_d"].numpy(), uv=r["uv"].numpy())
            only = scene.perspective_rendering(c2ws, intr, (H, W), render_latlong_map=True)
            fix["keys_latlong_without_uv"] = np.array(sorted(only.keys()))
            fix["keys_all_flags"] = np.array(sorted(r.keys()))
        fix["cubemap%d" % C], fix["latlong%d" % C], fix["images%d" % C] = cube.numpy(), lat.numpy(), images[C].numpy()
        fix["cubemap_attr%d" % C], fix["latlong_map_attr%d" % C] = r["cubemap_attr"].numpy(), r["latlong_map_attr"].numpy()
        tag[0] = "c2l%d_" % C
        fix["cubemap_to_latlong%d" % C] = R.cubemap_to_latlong(cube, (HT, WT)).numpy()
        inv = scene.perspective_inverse_rendering_torch(c2ws, intr, images[C], (H, W), (HT, WT), render_uv=True, render_latlong_map=True)
        fix["inv_latlong_map_attr%d" % C] = inv["latlong_map_attr"].numpy()
        assert (inv["latlong_map_attr"] == 0).any() and (inv["latlong_map_attr"] == 1).any(), "an unseen texel and the clamp both occur"
    try:
        scene.perspective_inverse_rendering_torch(c2ws, intr[None].expand(M, 3, 3), images[3], (H, W), (HT, WT), render_uv=True)
        fix["inverse_batched_intrinsics_fail"] = np.int32(0)
    except RuntimeError:
        fix["inverse_batched_intrinsics_fail"] = np.int32(1)
    cube3 = torch.from_numpy(fix["cubemap3"])
    fix["flatten"], fix["flatten_kjl"] = R.cubemap_to_flatten(cube3).numpy(), R.cubemap_to_flatten_kjl(cube3).numpy()
    fix["flatten_kjl_cubemap"] = R.flatten_to_cubemap(R.cubemap_to_flatten_kjl(cube3)).numpy()
    fix["grid_to_cube"] = R.grid_to_cube(torch.linspace(-0.75, 0.75, N)[None, :], torch.linspace(-0.75, 0.75, N)[:, None]).numpy()
    depth_map = torch.from_numpy(rng.uniform(0.5, 2.0, (HT, WT, 1)).astype(F32))
    fix["pcd_depth"], fix["pcd"] = depth_map.numpy(), R.latlong_depth_to_pcd(depth_map).numpy()
    fix.update(log)
    for k, v in fix.items():
        assert v.dtype.kind in "US" or np.isfinite(v).all(), k
    path = os.path.join(out, "g23_scene.npz")
    np.savez_compressed(path, **fix)
    print("G23: %d arrays, %d bytes, radius %.3f, seen %.3f, inside %.3f" % (len(fix), os.path.getsize(path), radius, seen.mean(), alpha.mean()))


def _dirs64():
    gx, gy = 2.0 * ((np.arange(WT) + 0.5) / WT) - 1.0, 2.0 * ((np.arange(HT) + 0.5) / HT) - 1.0
    psi, theta = (gx * np.pi)[None, :], (gy * (np.pi / 2) + np.pi / 2)[:, None]
    return np.stack(np.broadcast_arrays(np.sin(theta) * np.sin(psi), np.cos(theta), -np.sin(theta) * np.cos(psi)), -1)


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g23(out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
