#!/usr/bin/env python
"""Generate the 9-channel (PBR stack) back-projection fixture under tests/golden/ from the REFERENCE's own Python (mv_to_pcd, uv_to_pcd,
bake_mv_to_uv_reproject_blur), through the seams of make_golden.py and make_golden_reproject_variants.py (imported from there, unchanged):

    python tests/golden/make_golden_pbr_stack.py     # writes tests/golden/g67s_pbr_stack.npz

  G67s  the G67g scene (perspective box cameras at 2.8, fov 49.1, 48^2 views, a 96^2 atlas, the same holed view alpha) with views of NINE channels:
        three _views groups (albedo / metallic-roughness / bump stand-ins) of different seeds and frequencies.  One uv_to_pcd, then
        bake_mv_to_uv_reproject_blur(method='lens') and (method='gaussian') at the default sizes; plus one orthographic run sampled with
        grid_interpolate_mode='nvdiff' (the G67n 'o' cameras) through the lens bake.

The generator asserts, on the reference's output alone, that the three channel groups of color_2d differ from each other on more than 50 covered
texels: a build that copies group 0 cannot pass.  Masks are stored with np.packbits, the views as float16 (rounded to half first, so exact), the
atlases as float32."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _make_inverse_renderer, install_stubs  # noqa: E402
from make_golden_reproject_variants import _bake, _cameras, _uv, _views, install_variant_seams  # noqa: E402

GROUPS = ((41, 7, 5), (47, 5, 8), (53, 9, 3))      # (seed, fx, fy) per channel group; the first is G67g's


def _views9(HW):
    parts = [_views(HW, *g) for g in GROUPS]
    return np.concatenate([p[0] for p in parts], axis=-1), parts[0][1], parts[0][2]


def _assert_groups_differ(name, color_2d, cov):
    for a, b in ((0, 1), (0, 2), (1, 2)):
        d = int((np.abs(color_2d[0, ..., 3 * a:3 * a + 3] - color_2d[0, ..., 3 * b:3 * b + 3]).max(-1) > 1e-3)[cov].sum())
        print("G67s %s: groups %d and %d differ on %d covered texels" % (name, a, b, d))
        assert d > 50, "channel groups %d and %d of %s must differ on more than 50 covered texels" % (a, b, name)


def g67s_pbr_stack(out):
    inv, R, (verts, faces, uvs) = _make_inverse_renderer()
    HW, T = 48, 96
    imgs, xx, yy = _views9(HW)
    assert imgs.shape == (6, HW, HW, 9)
    fix = dict(verts=verts, faces=faces, uvs=uvs, images=imgs.astype(np.float16))
    # perspective, grid_sample: the G67g scene
    c2ws, intr = _cameras(2.8, True)
    hole = torch.from_numpy((((xx - 0.5) ** 2 + (yy - 0.5) ** 2) > 0.16 ** 2) | (xx < 0.3)).float()[None, :, :, None]
    with torch.no_grad():
        mv, alpha, uv = _uv(inv, c2ws, intr, imgs, hole, True, "torch", HW, T)
        cov = uv["mask_2d"].numpy()[0, ..., 0]
        c_l, _ = _bake(inv, uv, "lens")
        c_g, _ = _bake(inv, uv, "gaussian")
    assert c_l.shape == c_g.shape == (1, T, T, 9)
    _assert_groups_differ("lens", c_l, cov)
    _assert_groups_differ("gaussian", c_g, cov)
    assert (np.abs(c_l - c_g).max(-1) > 1e-4).sum() > 50, "the two blurs must differ on the seam"
    fix.update(c2ws=c2ws.numpy(), intr=intr.numpy(), alpha=np.packbits(alpha.numpy() > 0), mv_alpha=np.packbits(mv["alpha"].numpy() > 0),
               mask_2d=np.packbits(uv["mask_2d"].numpy()), mask_2d_visiable=np.packbits(uv["mask_2d_visiable"].numpy()),
               color_2d_lens=c_l, color_2d_gauss=c_g)
    # orthographic, nvdiffrast sampling: the G67n 'o' cameras and hole
    c2ws_o, intr_o = _cameras(2.8, False)
    hole_o = torch.from_numpy(((xx - 0.5) ** 2 + (yy - 0.5) ** 2) > 0.16 ** 2).float()[None, :, :, None]
    with torch.no_grad():
        mv_o, alpha_o, uv_o = _uv(inv, c2ws_o, intr_o, imgs, hole_o, False, "nvdiff", HW, T)
        c_o, _ = _bake(inv, uv_o, "lens")
    _assert_groups_differ("nvdiff", c_o, uv_o["mask_2d"].numpy()[0, ..., 0])
    fix.update(c2ws_o=c2ws_o.numpy(), intr_o=intr_o.numpy(), alpha_o=np.packbits(alpha_o.numpy() > 0), mv_alpha_o=np.packbits(mv_o["alpha"].numpy() > 0),
               mask_2d_visiable_o=np.packbits(uv_o["mask_2d_visiable"].numpy()), color_2d_nvdiff_o=c_o)
    path = os.path.join(out, "g67s_pbr_stack.npz")
    np.savez_compressed(path, **fix)
    size = os.path.getsize(path)
    if size > (1 << 20):      # the repository's cap on a committed file: drop the extra run first
        for k in ("c2ws_o", "intr_o", "alpha_o", "mv_alpha_o", "mask_2d_visiable_o", "color_2d_nvdiff_o"):
            fix.pop(k)
        np.savez_compressed(path, **fix)
        size = os.path.getsize(path)
        print("G67s: the orthographic nvdiff run is left out (file size)")
    assert size <= (1 << 20), size
    print("G67s: %d bytes" % size)


def main():
    sys.path.insert(0, REF)
    install_stubs()
    install_variant_seams()
    torch.set_num_threads(4)
    g67s_pbr_stack(HERE)
    print("wrote g67s_pbr_stack")


if __name__ == "__main__":
    main()
