"""The 9-channel (PBR stack) bake without a GPU: fixture G67s (tests/golden/make_golden_pbr_stack.py, the reference's own bake_mv_to_uv_reproject_blur on
nine channels) against the unchanged CPU oracle run PER CHANNEL GROUP, the GLB material round trip, and infer()'s channel-count checks."""
import json
import struct

import numpy as np
import pytest
import torch

from oracle import geom_ref as G
from oracle import reproject_ref as RV
from oracle.reproject_ref import HW, N, T, check_atlas, g67s, unpack

F32 = np.float32


def test_g67s_groups_differ():
    """what the generator asserts, once more on the committed file: a build that copies group 0 cannot pass"""
    f, imgs, _ = g67s()
    cov = unpack(f["mask_2d"], (1, T, T, 1))[0, ..., 0]
    for key in ("color_2d_lens", "color_2d_gauss"):
        c = f[key]
        assert c.shape == (1, T, T, 9) and c.dtype == F32
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert int((np.abs(c[0, ..., 3 * a:3 * a + 3] - c[0, ..., 3 * b:3 * b + 3]).max(-1) > 1e-3)[cov].sum()) > 50
    assert (np.abs(f["color_2d_lens"] - f["color_2d_gauss"]).max(-1) > 1e-4).sum() > 50


def test_g67s_oracle_per_group_reproduces_the_nine_channel_reference():
    """the reference's 9-channel bake IS the 3-channel bake per group: the unchanged oracle chain, run once per [group, alpha] image stack,
    reproduces color_2d of both blurs; visibility, which reads no colour, comes out the same for every group and within the oracle's cap of 4"""
    f, imgs, alpha = g67s()
    verts, faces, uvs, c2ws, intr = f["verts"], f["faces"], f["uvs"], f["c2ws"], f["intr"]
    s = RV.scene(dict(verts=verts, faces=faces, uvs=uvs, c2ws_p=c2ws, intr_p=intr), "p")
    mv_alpha = np.stack([G.rasterize(s["clip"][v], faces, HW, HW)[..., 3] > 0 for v in range(N)])
    assert np.array_equal(mv_alpha, unpack(f["mv_alpha"], (N, HW, HW, 1))[..., 0]), "view coverage"
    ref_vis = unpack(f["mask_2d_visiable"], (N, T, T, 1))[..., 0]
    cov_ref = unpack(f["mask_2d"], (1, T, T, 1))[0, ..., 0]
    got = {"lens": [], "gauss": []}
    vis0 = None
    for g in range(3):
        images4 = np.concatenate([imgs[..., 3 * g:3 * g + 3], alpha], -1)
        rast2d, rv, ao, col, vis = RV.texel_layers(s, T, images4, 100.0, "grid")
        cov = rast2d[..., 3] > 0
        assert np.array_equal(cov, cov_ref)
        if vis0 is None:
            vis0 = vis
            mism = int((vis.astype(bool) != ref_vis).sum())
            print("G67s oracle visibility: %d of %d texel-views differ" % (mism, ref_vis.size))
            assert mism <= 4
        assert np.array_equal(vis, vis0), "visibility does not depend on colour"
        atlas, seen, winner, bnd = G.composite(col, vis.astype(bool))
        filled, _ = G.nn_fill(atlas, seen, cov, G.interpolate(verts, rast2d, faces))
        seam = G.seam_mask(bnd, cov)
        for key, blur in (("lens", G.lens_blur_collapsed(filled, seam)), ("gauss", RV.gaussian_blur_fp64(filled, 5, seam).astype(F32))):
            got[key].append(G.pull_push(np.ascontiguousarray(blur.transpose(2, 0, 1), F32), cov).transpose(1, 2, 0))
    for key, name in (("lens", "color_2d_lens"), ("gauss", "color_2d_gauss")):
        ref = f[name][0]
        for g in range(3):
            check_atlas("G67s oracle %s group %d" % (key, g), got[key][g], ref[..., 3 * g:3 * g + 3])
        check_atlas("G67s oracle %s all nine" % key, np.concatenate(got[key], -1), ref)


def _glb_json(path):
    blob = open(path, "rb").read()
    clen, ctype = struct.unpack_from("<II", blob, 12)
    assert ctype == 0x4E4F534A
    return json.loads(blob[20:20 + clen].decode())


def test_glb_round_trip_with_the_pbr_material(tmp_path):
    from unitex_amd.texturetools import meshes
    verts, faces, uvs = meshes.sphere_with_faces(300)
    rng = np.random.default_rng(5)
    albedo, mr, bump = [(rng.random((24, 40, 3)) * 255).astype(np.uint8) for _ in range(3)]
    p = str(tmp_path / "pbr.glb")
    meshes.save_glb(p, verts, faces, uvs, albedo, metallic_roughness_u8=mr, bump_u8=bump)
    m = meshes.load_material_textures(p)
    assert np.array_equal(m["base_color"], albedo) and np.array_equal(m["metallic_roughness"], mr) and np.array_equal(m["normal"], bump)
    js = _glb_json(p)
    mat = js["materials"][0]
    assert mat == m["material"]
    pbr = mat["pbrMetallicRoughness"]
    assert pbr["baseColorTexture"] == {"index": 0} and pbr["metallicRoughnessTexture"] == {"index": 1} and mat["normalTexture"] == {"index": 2}
    for k in ("metallicFactor", "roughnessFactor", "baseColorFactor"):
        assert k not in pbr and k not in mat
    assert len(js["textures"]) == 3 and len(js["images"]) == 3
    # load_glb keeps its return shape and still finds the albedo
    v2, f2, uv2, tex = meshes.load_glb(p)
    assert np.array_equal(tex, albedo) and np.array_equal(f2, faces) and np.allclose(v2, verts)
    with pytest.raises(ValueError):
        meshes.save_glb(p, verts, faces, uvs, albedo, metallic_roughness_u8=mr)


def test_glb_without_the_extra_images_is_what_it_was(tmp_path):
    from unitex_amd.texturetools import meshes
    verts, faces, uvs = meshes.sphere_with_faces(300)
    albedo = (np.random.default_rng(6).random((16, 16, 3)) * 255).astype(np.uint8)
    p, q = str(tmp_path / "rgb.glb"), str(tmp_path / "rgb_none.glb")
    meshes.save_glb(p, verts, faces, uvs, albedo)
    meshes.save_glb(q, verts, faces, uvs, albedo, metallic_roughness_u8=None, bump_u8=None)
    assert open(p, "rb").read() == open(q, "rb").read()
    js = _glb_json(p)
    assert js["materials"] == [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0}}]
    assert js["textures"] == [{"source": 0, "sampler": 0}]
    assert js["images"] == [{"bufferView": 3, "mimeType": "image/png"}]
    assert list(js["materials"][0]["pbrMetallicRoughness"]) == ["baseColorTexture", "metallicFactor", "roughnessFactor"]
    assert len(js["bufferViews"]) == 4
    m = meshes.load_material_textures(p)
    assert np.array_equal(m["base_color"], albedo) and m["metallic_roughness"] is None and m["normal"] is None


def test_obj_export_of_a_pbr_mesh_names_three_images(tmp_path):
    from PIL import Image
    from unitex_amd.texturetools import meshes
    from unitex_amd.texturetools.renderer_inverse import TexturedMesh
    verts, faces, uvs = meshes.sphere_with_faces(300)
    rng = np.random.default_rng(7)
    albedo, mr, bump = [(rng.random((8, 8, 3)) * 255).astype(np.uint8) for _ in range(3)]
    TexturedMesh(verts, faces, uvs, albedo, mr, bump).export(str(tmp_path / "m.obj"))
    mtl = open(str(tmp_path / "m.mtl")).read()
    assert mtl == "newmtl material_0\nmap_Kd m.png\nmap_Pm m_metallic_roughness.png\nmap_Bump m_bump.png\n"
    for name, img in (("m.png", albedo), ("m_metallic_roughness.png", mr), ("m_bump.png", bump)):
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / name))), img)
    rgb = TexturedMesh(verts, faces, uvs, albedo)
    assert rgb.metallic_roughness is None and rgb.bump is None
    rgb.export(str(tmp_path / "r.obj"))
    assert open(str(tmp_path / "r.mtl")).read() == "newmtl material_0\nmap_Kd r.png\n"


def test_infer_channel_counts():
    """3 and 9 channels are accepted for both methods, anything else is refused with the reference's message (renderer_inverse.py:724); nine channels
    with return_layers=True are refused by name -- all before any device work"""
    from unitex_amd.texturetools import renderer_inverse as RI
    RI._check_channels((6, 8, 8, 3))
    RI._check_channels(torch.Size((6, 8, 8, 9)))
    inv = RI.NVDiffRendererInverse(device="cpu")
    c2ws = torch.eye(4)[None].repeat(6, 1, 1)
    for C in (4, 1, 6, 12):
        for method in ("reproject", "kdtree"):
            with pytest.raises(NotImplementedError) as e:
                inv.infer(None, c2ws=c2ws, intrinsics=torch.eye(3), image_attrs=torch.zeros(6, 8, 8, C), method=method)
            assert str(e.value) == "shape torch.Size([6, 8, 8, %d]) is not supported" % C
    with pytest.raises(NotImplementedError, match="return_layers"):
        inv.infer(None, c2ws=c2ws, intrinsics=torch.eye(3), image_attrs=torch.zeros(6, 8, 8, 9), method="reproject", return_layers=True)


def test_oracle_push_at_an_odd_size_is_the_replicate_padded_upsample():
    """the reference stops at odd sizes, so G._push is the only statement of what the push kernel does there; it is held to values worked out by hand.
    Bilinear 2x upsampling is separable, and along one axis a replicate-padded mip (v0, v1) gives the five fine texels v0, (3 v0 + v1) / 4, (v0 + 3 v1) / 4,
    v1 and, for the fifth, whose near cell is the padding, v1 again: up = U mip U^T.  Every product below is exact in fp32.  An upsample that gave the last
    row the cells (1, 0) as near and far instead would repeat row 2 there."""
    mip = np.array([[[0, 16], [32, 64]]], F32)
    want = np.array([[0, 4, 12, 16, 16],
                     [8, 13, 23, 28, 28],
                     [24, 31, 45, 52, 52],
                     [32, 40, 56, 64, 64],
                     [32, 40, 56, 64, 64]], F32)
    U = np.array([[1, 0], [0.75, 0.25], [0.25, 0.75], [0, 1], [0, 1]], np.float64)
    assert np.array_equal(want, U @ mip[0].astype(np.float64) @ U.T)
    kd = np.full((1, 5, 5), -1, F32)
    mask = np.zeros((5, 5), bool)
    mask[1, 3] = mask[4, 4] = True                  # covered texels keep their own value
    got, m = G._push(kd, mask, mip, np.ones((2, 2), bool))
    want[1, 3] = want[4, 4] = -1
    assert np.array_equal(got[0], want) and m is mask
    # the pull drops the odd last row / column, as avg_pool2d does
    k5 = np.arange(25, dtype=F32).reshape(1, 5, 5)
    k, a = G._pull(k5, np.ones((5, 5), bool))
    assert np.array_equal(k[0], np.array([[3, 5], [13, 15]], F32)) and a.shape == (2, 2) and a.all()
