"""The 9-channel (PBR stack) bake on the GPU: fixture G67s through NVDiffRendererInverse.infer against the reference's own outputs, bit-identity of the
9-channel path against the 3-channel path per channel group, the post-processing stages at C channels against their thread-per-texel instantiation
(C = 3) and against the numpy restatement, the new entry points alone, view sharding, the PBR TexturedMesh and its GLB, and the refusals."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import reproject_ref as RV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
N, HW, T = RV.N, RV.HW, RV.T


def _infer(f, images, alpha, c2ws, intr, method="reproject", return_layers=False, **kw):
    """infer() on a G67-style fixture; the view alpha the generator holed is substituted at the mv_to_pcd seam, as in test_reproject_variants_gpu._infer"""
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse

    class Inv(NVDiffRendererInverse):
        def mv_to_pcd(self, *a, **k):
            out = super().mv_to_pcd(*a, **k)
            out["alpha"] = torch.from_numpy(alpha).to(out["alpha"].device).contiguous()
            return out
    inv = Inv(device="cuda").update_from_arrays(f["verts"], f["faces"], f["uvs"])
    out = inv.infer(None, c2ws=c2ws, intrinsics=intr, image_attrs=torch.from_numpy(images), H=images.shape[1], W=images.shape[2], H2D=T, W2D=T,
                    ray_normal_angle_threhold=100.0, method=method, filt_gradient_points=False, return_layers=return_layers, **kw)
    torch.cuda.synchronize()
    return inv, out


# ------------------------------------------------------------------------------------------------ 1. the fixture through infer
@pytest.mark.parametrize("blur,key", [("lens", "color_2d_lens"), ("gaussian", "color_2d_gauss")])
def test_g67s_fixture_through_infer(blur, key):
    f, imgs, alpha = RV.g67s()
    inv, (textured, mask_vis, mask_2d, color_2d) = _infer(f, imgs, alpha[..., 0], f["c2ws"], f["intr"], perspective=True, reproject_method=blur)
    assert tuple(color_2d.shape) == (1, T, T, 9)
    assert np.array_equal(mask_2d.cpu().numpy()[0, ..., 0], RV.unpack(f["mask_2d"], (1, T, T, 1))[0, ..., 0])
    got_vis, ref_vis = mask_vis.cpu().numpy()[..., 0], RV.unpack(f["mask_2d_visiable"], (N, T, T, 1))[..., 0]
    mism = int((got_vis != ref_vis).sum())
    print("G67s %s visibility: %d of %d texel-views differ" % (blur, mism, ref_vis.size))
    assert mism <= 2
    got, ref = color_2d.cpu().numpy()[0], f[key][0]
    for g in range(3):
        RV.check_atlas("G67s %s group %d" % (blur, g), got[..., 3 * g:3 * g + 3], ref[..., 3 * g:3 * g + 3])
    RV.check_atlas("G67s %s all nine" % blur, got, ref)


# ------------------------------------------------------------------------------------------------ 2. bit-identity against the 3-channel path
def _assert_groups_equal_the_rgb_path(run, imgs9, what):
    inv9, out9 = run(imgs9)
    assert tuple(out9[3].shape[-1:]) == (9,)
    for g in range(3):
        inv3, out3 = run(np.ascontiguousarray(imgs9[..., 3 * g:3 * g + 3]))
        assert torch.equal(out9[3][..., 3 * g:3 * g + 3], out3[3]), "%s: color_2d of group %d differs from the 3-channel path" % (what, g)
        assert torch.equal(out9[1], out3[1]), "%s: mask_2d_visiable" % what
        assert torch.equal(inv9.last["winner"], inv3.last["winner"]) and torch.equal(inv9.last["seam"], inv3.last["seam"]), "%s: winner / seam" % what
        assert torch.equal(inv9.last["atlas_prefill"][..., 3 * g:3 * g + 3], inv3.last["atlas_prefill"]), "%s: the atlas before pull-push" % what
    assert inv9.last["seam"].any() and (inv9.last["winner"] < 0).any() and (inv9.last["winner"] >= 0).any()
    assert not torch.equal(out9[3][..., 0:3], out9[3][..., 3:6]) and not torch.equal(out9[3][..., 3:6], out9[3][..., 6:9])


VARIANTS = [dict(), dict(reproject_method="gaussian"), dict(grid_interpolate_mode="nvdiff"),
            dict(reproject_method="gaussian", grid_interpolate_mode="nvdiff", reproject_kernel_size_boundary=5, reproject_kernel_size_boundary_blur=5,
                 reproject_kernel_size_blur=7),
            dict(reproject_kernel_size_boundary=7, reproject_kernel_size_boundary_blur=1)]


@pytest.mark.parametrize("persp", [True, False])
@pytest.mark.parametrize("vi", range(len(VARIANTS)))
def test_nine_channels_equal_three_rgb_bakes_bit_for_bit_on_the_fixture_scene(persp, vi):
    from unitex_amd.texturetools import camera
    f, imgs, alpha = RV.g67s()
    if persp:
        c2ws, intr = f["c2ws"], f["intr"]
    else:
        c2ws, intr = f["c2ws"], camera.generate_intrinsics(1.0, 1.0, fov=False)
    kw = VARIANTS[vi]
    _assert_groups_equal_the_rgb_path(lambda im: _infer(f, im, alpha[..., 0], c2ws, intr, perspective=persp, **kw), imgs, "G67s scene %s %r" % (persp, kw))


def _views9(n, px):
    """nine smooth channels: three smooth_views groups, the second and third mirrored and inverted so that the groups differ"""
    from unitex_amd.texturetools.benchmarks import smooth_views
    a = smooth_views(n, px, px)
    return np.ascontiguousarray(np.concatenate([a, a[:, ::-1, :, ::-1], 1.0 - a[:, :, ::-1]], -1), F32)


@pytest.mark.parametrize("persp,kw", [(False, dict()), (True, dict(reproject_method="gaussian", grid_interpolate_mode="nvdiff", reproject_kernel_size_boundary=5))])
def test_nine_channels_equal_three_rgb_bakes_bit_for_bit_at_scale(persp, kw):
    """the 50 k-face sphere at 6 x 512^2 -> 2048^2, with the gradient filter on (the pipeline's setting)"""
    from unitex_amd.texturetools import camera, meshes
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    verts, faces, uvs = meshes.sphere_with_faces(50000)
    c2ws = camera.generate_box_views_c2ws(2.8)[[0, 1, 4, 2, 3, 5]]
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True) if persp else camera.generate_intrinsics(1.0, 1.0, fov=False)
    imgs = _views9(6, 512)
    inv = NVDiffRendererInverse(device="cuda").update_from_arrays(verts, faces, uvs)

    def run(im):
        out = inv.infer(None, c2ws=c2ws, intrinsics=intr, image_attrs=torch.from_numpy(im), perspective=persp, H=512, W=512, H2D=2048, W2D=2048,
                        filt_gradient_points=True, **kw)
        torch.cuda.synchronize()

        class Last:
            last = dict(inv.last)
        return Last, out
    _assert_groups_equal_the_rgb_path(run, imgs, "50k sphere %s %r" % (persp, kw))


# ------------------------------------------------------------------------------------------------ 3. the entry points alone
def _scene(persp, n_faces=20000, px=128, Tt=256):
    from unitex_amd.texturetools import camera, meshes, ops
    from unitex_amd.texturetools.benchmarks import smooth_views
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    verts, faces, uvs = meshes.sphere_with_faces(n_faces)
    inv = NVDiffRendererInverse(device="cuda").update_from_arrays(verts, faces, uvs)
    c2ws = camera.generate_box_views_c2ws(1.8 if persp else 2.8)[[0, 1, 4, 2, 3, 5]]
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True) if persp else camera.generate_intrinsics(1.15, 1.15, fov=False)
    mv = inv.mv_to_pcd(c2ws, intr, (px, px), perspective=persp, filt_gradient_points=True)
    m = inv.pbr_mesh
    uvclip = torch.cat([m.uvs_2d, torch.zeros_like(m.uvs_2d[:, :1]), torch.ones_like(m.uvs_2d[:, :1])], dim=-1).contiguous()
    rast2d = ops.rasterize(uvclip, m.faces, *((Tt, Tt) if isinstance(Tt, int) else Tt))
    c2 = torch.as_tensor(c2ws, dtype=torch.float32)
    eyes = c2[:, :3, 3].contiguous().cuda() if persp else None
    dirs = None if persp else (-c2[:, :3, 2]).contiguous().cuda()
    rgb = torch.from_numpy(smooth_views(6, px, px)).cuda()
    return dict(m=m, rast2d=rast2d, vndc=mv["ndc"].contiguous(), alpha=mv["alpha"].contiguous(), eyes=eyes, dirs=dirs, rgb=rgb, bvh=m.optix,
                view_dirs=(-c2[:, :3, 2]).contiguous())


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("sample", ["grid", "nvdiff"])
def test_backproject_vis_equals_the_colour_kernel_on_all_traversal_modes(persp, sample):
    from unitex_amd import _lib
    from unitex_amd.texturetools import ops
    s = _scene(persp)
    m = s["m"]
    images4 = torch.cat([s["rgb"], s["alpha"][..., None]], -1).contiguous()
    before = _lib.get_options()
    seen = []
    try:
        for packet, stack in ((1, 0), (0, 0), (0, 1)):      # packet walk, packed thread-per-ray walk, stack walk
            _lib.set_option("UTX_BVH_PACKET", packet)
            _lib.set_option("UTX_BVH_STACK_WALK", stack)
            _, rv, ao = ops.backproject(s["rast2d"], m.vertices, m.faces, m.normals, s["vndc"], s["dirs"], images4, s["bvh"], eyes=s["eyes"], sample=sample)
            rv2, ao2 = ops.backproject_vis(s["rast2d"], m.vertices, m.faces, m.normals, s["vndc"], s["dirs"], s["alpha"], s["bvh"], eyes=s["eyes"], sample=sample)
            torch.cuda.synchronize()
            assert torch.equal(rv, rv2) and torch.equal(ao, ao2), "mode packet=%d stack=%d" % (packet, stack)
            seen.append(rv)
    finally:
        _lib.set_option("UTX_BVH_PACKET", before["UTX_BVH_PACKET"])
        _lib.set_option("UTX_BVH_STACK_WALK", before["UTX_BVH_STACK_WALK"])
    assert seen[0].any() and not seen[0].all() and ao.any() and not ao.all()
    # a view block: the other views' layers are left alone
    rv3 = torch.full_like(rv, 7)
    ao3 = torch.full_like(ao, 7)
    ops.backproject_vis(s["rast2d"], m.vertices, m.faces, m.normals, s["vndc"], s["dirs"], s["alpha"], s["bvh"], eyes=s["eyes"], sample=sample,
                        view_begin=2, view_count=3, out=(rv3, ao3))
    assert torch.equal(rv3[2:5], seen[0][2:5]) and bool((rv3[:2] == 7).all()) and bool((rv3[5:] == 7).all()) and torch.equal(ao3[2:5], ao[2:5])


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("sample", ["grid", "nvdiff"])
def test_gather_winner_at_three_channels_equals_composite_of_backproject(persp, sample):
    from unitex_amd.texturetools import ops
    from unitex_amd.texturetools.renderer_inverse import PRIORITY
    s = _scene(persp)
    m = s["m"]
    images4 = torch.cat([s["rgb"], s["alpha"][..., None]], -1).contiguous()
    col, rv, ao = ops.backproject(s["rast2d"], m.vertices, m.faces, m.normals, s["vndc"], s["dirs"], images4, s["bvh"], eyes=s["eyes"], sample=sample)
    vis = ops.dilate_visibility(rv, ao, s["rast2d"])
    atlas, winner = ops.composite(col, vis, PRIORITY)
    w2 = ops.composite_winner(vis, PRIORITY)
    assert torch.equal(winner, w2)
    got = ops.gather_winner(s["rast2d"], m.faces, s["vndc"], s["rgb"].contiguous(), w2, sample=sample)
    assert torch.equal(got, atlas)
    assert (winner >= 0).any() and (winner < 0).any() and atlas.abs().sum() > 0
    # other channel counts: every channel is sampled as channel (c % 3) of the rgb gather
    for Cc in (1, 9, 16):
        idx = [c % 3 for c in range(Cc)]
        g = ops.gather_winner(s["rast2d"], m.faces, s["vndc"], s["rgb"][..., idx].contiguous(), w2, sample=sample)
        assert torch.equal(g, atlas[..., idx])
    # the reversed order: the winner changes exactly where more than one view sees a texel
    order = PRIORITY[::-1]
    a3, w3 = ops.composite(col, vis, order)
    assert torch.equal(ops.composite_winner(vis, order), w3)
    assert torch.equal(w3 != winner, vis.sum(0) > 1)
    assert torch.equal(ops.gather_winner(s["rast2d"], m.faces, s["vndc"], s["rgb"].contiguous(), w3, sample=sample), a3)


@functools.lru_cache(maxsize=None)
def _border_scene(persp):
    """a 2 000-face sphere, six 64 x 64 views, an atlas of 80 rows x 96 columns, and every view's vertex NDC multiplied by 1.6: part of the surface projects
    outside the view, so the zero-padded taps of the grid mode and the wrap of the nvdiff mode run.  Built once per camera model, never written to."""
    s = _scene(persp, n_faces=2000, px=64, Tt=(80, 96))
    s["vndc"] = (s["vndc"] * 1.6).contiguous()
    return s


@pytest.mark.parametrize("persp", [False, True])
@pytest.mark.parametrize("sample", ["grid", "nvdiff"])
def test_the_three_sampling_kernels_agree_where_the_surface_leaves_the_view(persp, sample):
    """backproject, backproject_vis and gather_winner share one statement of each sampling mode; the scenes of the tests above keep the whole mesh inside
    every view, this one does not.  Everything bit for bit; the grid mode also against the oracle's gather (its rays are orthographic, so the perspective
    case compares the ray-independent outputs, as test_perspective_gpu.py does)."""
    from oracle import geom_ref as G
    from unitex_amd.texturetools import ops
    from unitex_amd.texturetools.renderer_inverse import PRIORITY
    s = _border_scene(persp)
    m = s["m"]
    assert tuple(s["rast2d"].shape) == (80, 96, 4)
    # the guard: covered texels project both outside and inside the view
    covered = s["rast2d"][..., 3] > 0
    reach = torch.stack([ops.interpolate(s["vndc"][v].contiguous(), s["rast2d"], m.faces).abs().amax(-1) for v in range(6)])
    outside, inside = (reach > 1)[:, covered], (reach < 1)[:, covered]
    print("covered texel-views with |ndc| > 1: %d, with |ndc| < 1: %d" % (int(outside.sum()), int(inside.sum())))
    assert bool(outside.any()) and bool(inside.any())
    images4 = torch.cat([s["rgb"], s["alpha"][..., None]], -1).contiguous()
    col, rv, ao = ops.backproject(s["rast2d"], m.vertices, m.faces, m.normals, s["vndc"], s["dirs"], images4, s["bvh"], eyes=s["eyes"], sample=sample)
    rv2, ao2 = ops.backproject_vis(s["rast2d"], m.vertices, m.faces, m.normals, s["vndc"], s["dirs"], s["alpha"], s["bvh"], eyes=s["eyes"], sample=sample)
    assert torch.equal(rv, rv2) and torch.equal(ao, ao2)
    assert rv.any() and not rv.all() and ao.any() and not ao.all()
    vis = ops.dilate_visibility(rv, ao, s["rast2d"])
    atlas, winner = ops.composite(col, vis, PRIORITY)
    assert torch.equal(ops.composite_winner(vis, PRIORITY), winner)
    assert (winner >= 0).any() and (winner < 0).any() and atlas.abs().sum() > 0
    for Cc in (3, 1, 9):
        idx = [c % 3 for c in range(Cc)]
        got = ops.gather_winner(s["rast2d"], m.faces, s["vndc"], s["rgb"][..., idx].contiguous(), winner, sample=sample)
        assert torch.equal(got, atlas[..., idx]), "gather_winner at C = %d" % Cc
    if sample == "grid":
        verts, faces = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
        col_ref, rv_ref, ao_ref = G.backproject(s["rast2d"].cpu().numpy(), verts, faces, m.normals.cpu().numpy(), s["vndc"].cpu().numpy(),
                                                s["view_dirs"].numpy(), images4.cpu().numpy(), G.BVH(verts, faces))
        assert np.array_equal(col.cpu().numpy(), col_ref) and np.array_equal(ao.cpu().numpy(), ao_ref)
        if not persp:
            assert np.array_equal(rv.cpu().numpy(), rv_ref)


def _post_inputs(Hh, Ww, seed):
    """an atlas of 3 random channels with blobs of winners / unseen texels, a seam and coverage with holes"""
    from unitex_amd.texturetools import ops
    winner, rast2d = [t.cuda().contiguous() for t in RV._blob_winner(Hh, Ww, seed, 40)]
    seam = ops.seam_mask(winner, rast2d)
    g = torch.Generator().manual_seed(seed)
    atlas3 = torch.rand(Hh, Ww, 3, generator=g).cuda()
    pos = (torch.rand(Hh, Ww, 3, generator=g) * 2 - 1).cuda()
    return winner, rast2d, seam, atlas3, pos


@pytest.mark.parametrize("Cc", [1, 3, 9, 16])
@pytest.mark.parametrize("size", [(96, 160), (250, 131)])
def test_c_channel_post_processing_equals_the_three_channel_kernels_per_group(Cc, size):
    """ragged C is padded by repeating channels: C-channel input channel c holds base channel (c % 7) of a 7-channel base, and every group of three of the
    result (the last one padded by repeating) must equal the C = 3 result (the thread-per-texel instantiation) on those three channels"""
    from unitex_amd.texturetools import ops
    Hh, Ww = size
    winner, rast2d, seam, _, pos = _post_inputs(Hh, Ww, 11 + Cc)
    g = torch.Generator().manual_seed(100 + Cc)
    base = torch.rand(Hh, Ww, 7, generator=g).cuda()
    base = base * (winner >= 0)[..., None]        # the composite leaves zeros where no view sees the texel
    src = base[..., [c % 7 for c in range(Cc)]].contiguous()
    mask = (rast2d[..., 3] > 0).to(torch.uint8).contiguous()
    assert seam.any() and (winner < 0).any() and (mask == 0).any()

    def groups():
        for c0 in range(0, Cc, 3):
            ch = [min(c0 + j, Cc - 1) for j in range(3)]      # the ragged tail repeats its last channel
            yield ch
    # nn fill
    filled = src.clone()
    idx = ops.nn_fill(filled, winner, rast2d, pos, want_index=True)
    for ch in groups():
        a3 = src[..., ch].contiguous()
        idx3 = ops.nn_fill(a3, winner, rast2d, pos, want_index=True)
        assert torch.equal(filled[..., ch], a3) and torch.equal(idx, idx3)
    assert not torch.equal(filled, src)
    # the two blurs
    lens = ops.lens_blur_seam(filled, seam)
    gauss = {k: ops.gaussian_blur_seam(filled, seam, k) for k in (5, 7, 31)}
    for ch in groups():
        f3 = filled[..., ch].contiguous()
        assert torch.equal(lens[..., ch], ops.lens_blur_seam(f3, seam))
        for k in gauss:
            assert torch.equal(gauss[k][..., ch], ops.gaussian_blur_seam(f3, seam, k)), "gaussian %d" % k
    assert not torch.equal(lens, filled) and not torch.equal(gauss[5], lens)
    # pull-push
    pp = ops.pull_push(lens, mask)
    for ch in groups():
        assert torch.equal(pp[..., ch], ops.pull_push(lens[..., ch].contiguous(), mask))
    assert not torch.equal(pp, lens)


@pytest.mark.parametrize("Cc", [1, 9, 16])
@pytest.mark.parametrize("size", [(96, 160), (250, 131)])
def test_c_channel_post_processing_equals_the_numpy_restatement(Cc, size):
    """the two instantiations of a stage share one body, so the C-channel results are also held against oracle/geom_ref.py, at the tolerances the 3-channel
    chain has in test_geometry_gpu.py and test_reproject_variants_gpu.py: NN fill and pull-push exact, lens blur 2e-6 (libm's powf against the device's),
    Gaussian blur 1e-6 from the fp64 sum"""
    from oracle import geom_ref as G
    from unitex_amd.texturetools import ops
    Hh, Ww = size
    winner, rast2d, seam, _, pos = _post_inputs(Hh, Ww, 11 + Cc)
    src = torch.rand(Hh, Ww, Cc, generator=torch.Generator().manual_seed(200 + Cc)).cuda() * (winner >= 0)[..., None]
    mask = (rast2d[..., 3] > 0).to(torch.uint8).contiguous()
    unseen = (winner < 0) & (mask > 0)
    assert seam.any() and unseen.any() and (mask == 0).any()
    w_np, r_np, pos_np, seam_np, src_np = winner.cpu().numpy(), rast2d.cpu().numpy(), pos.cpu().numpy(), seam.cpu().numpy().astype(bool), src.cpu().numpy()
    # nn fill: the brute-force search takes three channels at a time
    filled = src.clone()
    idx = ops.nn_fill(filled, winner, rast2d, pos, want_index=True).cpu().numpy().reshape(Hh, Ww)
    filled_np = filled.cpu().numpy()
    for c0 in range(0, Cc, 3):
        ch = [min(c0 + j, Cc - 1) for j in range(3)]
        ref, idx_ref = G.nn_fill_brute(np.ascontiguousarray(src_np[..., ch]), w_np, r_np, pos_np)
        assert np.array_equal(idx, idx_ref) and np.array_equal(filled_np[..., ch], ref)
    assert (idx[unseen.cpu().numpy()] >= 0).all() and not np.array_equal(filled_np, src_np)
    # the two blurs
    lens = ops.lens_blur_seam(filled, seam)
    err = np.abs(lens.cpu().numpy() - G.lens_blur_collapsed(filled_np, seam_np)).max()
    print("C %d %s lens: max |d| %.3g" % (Cc, size, err))
    assert err < 2e-6
    for k in (5, 7, 31):
        err = np.abs(ops.gaussian_blur_seam(filled, seam, k).cpu().numpy() - RV.gaussian_blur_fp64(filled_np, k, seam_np)).max()
        print("C %d %s gaussian %d: max |d| %.3g" % (Cc, size, k, err))
        assert err <= 1e-6
    # pull-push, with holes over the last rows and columns as well: at an odd size the last row / column of a level lies past the last coarse cell, and the
    # push writes there only where that level is uncovered
    pp_mask = mask.clone()
    pp_mask[-6:, :] = 0
    pp_mask[:, -5:] = 0
    m0 = pp_mask.cpu().numpy().astype(bool)
    lens_np = np.ascontiguousarray(lens.cpu().numpy().transpose(2, 0, 1))
    _, m1 = G._pull(lens_np, m0)
    for m in (m0, m1):          # levels 0 and 1: 250 x 131 and 125 x 65
        assert not m[-1].any() and not m[:, -1].any()
    assert m0.any()
    pp = ops.pull_push(lens, pp_mask).cpu().numpy()
    pp_ref = G.pull_push(lens_np, m0).transpose(1, 2, 0)
    assert np.array_equal(pp, pp_ref) and not np.array_equal(pp, lens.cpu().numpy())


def test_pull_push_c_below_the_first_level_is_a_copy():
    from unitex_amd.texturetools import ops
    kd = torch.rand(7, 6, 9).cuda()
    mask = (torch.rand(7, 6) > 0.5).to(torch.uint8).cuda()
    assert torch.equal(ops.pull_push(kd, mask), kd)


# ------------------------------------------------------------------------------------------------ 4. view sharding
def _sharded_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from unitex_amd.texturetools import camera, meshes
        from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
        dev = "cuda:0"
        torch.cuda.set_device(0)
        verts, faces, uvs = meshes.sphere_with_faces(20000)
        c2ws = camera.generate_box_views_c2ws(1.8)[[0, 1, 4, 2, 3, 5]]
        intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
        images = torch.from_numpy(_views9(6, 256)).to(dev)
        kw = dict(c2ws=c2ws, intrinsics=intr, image_attrs=images, perspective=True, H=256, W=256, H2D=512, W2D=512,
                  filt_gradient_points=True, ray_normal_angle_threhold=115.0, grid_interpolate_mode="nvdiff",
                  reproject_method="gaussian", reproject_kernel_size_boundary=5, reproject_kernel_size_blur=7)
        inv = NVDiffRendererInverse(device=dev, view_shard=(rank, world)).update_from_arrays(verts, faces, uvs)
        out = inv.infer(None, **kw)
        torch.cuda.synchronize()
        res = {"rank": rank}
        if rank == 0:
            one = NVDiffRendererInverse(device=dev).update_from_arrays(verts, faces, uvs)
            ref = one.infer(None, **kw)
            torch.cuda.synchronize()
            res["channels"] = int(out[3].shape[-1])
            res["texture_equal"] = bool(np.array_equal(out[0].texture, ref[0].texture) and np.array_equal(out[0].metallic_roughness, ref[0].metallic_roughness)
                                        and np.array_equal(out[0].bump, ref[0].bump))
            res["color2d_equal"] = bool(torch.equal(out[3], ref[3]))
            res["vis_equal"] = bool(torch.equal(out[1], ref[1]))
            res["winner_equal"] = bool(torch.equal(inv.last["winner"], one.last["winner"]))
            res["seam_equal"] = bool(torch.equal(inv.last["seam"], one.last["seam"]))
            res["seam"] = float(one.last["seam"].float().mean())
        dist.barrier()
        if rank == 0:
            q.put(res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_view_sharded_nine_channel_infer_is_bit_identical_to_one_rank(world):
    """gloo ranks on one GPU, each back-projecting its block of the views; only the u8 visibility layers are exchanged"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + 40 * world + (os.getpid() % 30)
    procs = [ctx.Process(target=_sharded_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res["seam"] > 0.001 and res["channels"] == 9
    for k, v in res.items():
        if k.endswith("_equal"):
            assert v, "%s differs between world=%d and world=1: %s" % (k, world, res)


# ------------------------------------------------------------------------------------------------ 5. the mesh that comes out
@pytest.mark.parametrize("method", ["reproject", "kdtree"])
def test_nine_channel_infer_returns_a_pbr_mesh(method, tmp_path):
    from unitex_amd.texturetools import meshes, ops
    f, imgs, alpha = RV.g67s()
    inv, (textured, mask_vis, mask_2d, color_2d) = _infer(f, imgs, alpha[..., 0], f["c2ws"], f["intr"], method=method, perspective=True)
    assert tuple(color_2d.shape) == (1, T, T, 9)
    want = [ops.to_u8(color_2d[0, ..., 3 * g:3 * g + 3].contiguous(), flip=True).cpu().numpy() for g in range(3)]
    assert textured.texture.dtype == np.uint8 and np.array_equal(textured.texture, want[0])
    assert np.array_equal(textured.metallic_roughness, want[1]) and np.array_equal(textured.bump, want[2])
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
    p = textured.export(str(tmp_path / "x.glb"))
    m = meshes.load_material_textures(p)
    assert np.array_equal(m["base_color"], want[0]) and np.array_equal(m["metallic_roughness"], want[1]) and np.array_equal(m["normal"], want[2])
    pbr = m["material"]["pbrMetallicRoughness"]
    assert "metallicFactor" not in pbr and "roughnessFactor" not in pbr and "baseColorFactor" not in pbr
    assert np.array_equal(meshes.load_glb(p)[3], want[0])


def test_three_channel_infer_returns_an_rgb_mesh(tmp_path):
    from unitex_amd.texturetools import meshes
    f, imgs, alpha = RV.g67s()
    for method in ("reproject", "kdtree"):
        _, (textured, _, _, color_2d) = _infer(f, np.ascontiguousarray(imgs[..., :3]), alpha[..., 0], f["c2ws"], f["intr"], method=method, perspective=True)
        assert textured.metallic_roughness is None and textured.bump is None and color_2d.shape[-1] == 3
    m = meshes.load_material_textures(textured.export(str(tmp_path / "rgb.glb")))
    assert m["metallic_roughness"] is None and m["normal"] is None and m["material"]["pbrMetallicRoughness"]["metallicFactor"] == 0.0


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    from unitex_amd._lib import BackprojectDesc, ptr
    from unitex_amd.flux.ops import get_ctx
    from unitex_amd.texturetools import ops
    f, imgs, alpha = RV.g67s()
    with pytest.raises(NotImplementedError, match="return_layers"):
        _infer(f, imgs, alpha[..., 0], f["c2ws"], f["intr"], perspective=True, return_layers=True)
    with pytest.raises(NotImplementedError, match="is not supported"):
        _infer(f, np.ascontiguousarray(imgs[..., :4]), alpha[..., 0], f["c2ws"], f["intr"], perspective=True)
    # kdtree keeps its layers
    assert len(_infer(f, imgs, alpha[..., 0], f["c2ws"], f["intr"], method="kdtree", perspective=True, return_layers=True)[1]) == 6
    ctx = get_ctx(0)
    lib, h, st = ctx.lib, ctx.handle, ctx.stream()
    Hh = Ww = 16
    w = torch.zeros(Hh, Ww, dtype=torch.int8, device="cuda")
    r = torch.zeros(Hh, Ww, 4, device="cuda")
    faces = torch.zeros(1, 3, dtype=torch.int32, device="cuda")
    vndc = torch.zeros(6, 3, 2, device="cuda")
    img17 = torch.zeros(6, 4, 4, 17, device="cuda")
    a17 = torch.zeros(Hh, Ww, 17, device="cuda")
    seam = torch.zeros(Hh, Ww, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(Hh * Ww, dtype=torch.int32, device="cuda")
    work = torch.zeros(int(lib.utx_nn_fill_workspace_bytes(Hh * Ww)), dtype=torch.uint8, device="cuda")
    k49 = (C.c_float * 49)()
    w1 = (C.c_float * 5)()
    for Cc in (17, 0, -1):      # refused with -2 before any launch
        assert lib.utx_gather_winner(h, ptr(r), ptr(faces), ptr(vndc), ptr(img17), ptr(w), Hh * Ww, 3, 6, 4, 4, Cc, 0, ptr(a17), st) == -2
        assert lib.utx_nn_fill_c(h, ptr(r), ptr(w), ptr(r), Hh * Ww, Cc, ptr(a17), ptr(idx), ptr(work), work.numel(), st) == -2
        assert lib.utx_lens_blur_seam_c(h, ptr(a17), ptr(seam), Hh, Ww, Cc, k49, ptr(a17), st) == -2
        assert lib.utx_gaussian_blur_seam_c(h, ptr(a17), ptr(seam), Hh, Ww, Cc, 5, w1, ptr(a17), st) == -2
        assert lib.utx_pull_push_c(h, ptr(a17), ptr(seam), Hh, Ww, Cc, ptr(a17), ptr(work), st) == -2
        assert lib.utx_pull_push_workspace_bytes_c(Hh, Ww, Cc) == 0
    assert lib.utx_pull_push_workspace_bytes_c(Hh, Ww, 3) == lib.utx_pull_push_workspace_bytes(Hh, Ww)
    # null pointers, a bad sample mode, a bad order
    assert lib.utx_gather_winner(h, ptr(r), ptr(faces), ptr(vndc), None, ptr(w), Hh * Ww, 3, 6, 4, 4, 9, 0, ptr(a17), st) == -2
    assert lib.utx_gather_winner(h, ptr(r), ptr(faces), ptr(vndc), ptr(img17), ptr(w), Hh * Ww, 3, 6, 4, 4, 9, 2, ptr(a17), st) == -2
    assert lib.utx_nn_fill_c(h, ptr(r), ptr(w), ptr(r), Hh * Ww, 9, ptr(a17), None, ptr(work), work.numel(), st) == -2
    assert lib.utx_gaussian_blur_seam_c(h, ptr(a17), ptr(seam), Hh, Ww, 9, 4, w1, ptr(a17), st) == -2
    vis = torch.zeros(6, Hh, Ww, dtype=torch.uint8, device="cuda")
    bad = (C.c_int * 6)(0, 1, 2, 3, 4, 6)
    assert lib.utx_composite_winner(h, ptr(vis), 6, bad, 6, Hh * Ww, ptr(w), st) == -2
    assert lib.utx_composite_winner(h, None, 6, bad, 6, Hh * Ww, ptr(w), st) == -2
    s = _scene(False, n_faces=2000, px=32, Tt=32)
    d = BackprojectDesc()
    m = s["m"]
    d.rast2d, d.verts, d.faces, d.fnormal, d.vndc, d.dirs = ptr(s["rast2d"]), ptr(m.vertices), ptr(m.faces), ptr(m.normals), ptr(s["vndc"]), ptr(s["dirs"])
    rv = torch.zeros(6, 32, 32, dtype=torch.uint8, device="cuda")
    d.rayvis, d.alphaok = ptr(rv), ptr(rv.clone())
    d.T_h, d.T_w, d.V, d.n_views, d.H, d.W, d.view_begin, d.view_count = 32, 32, m.vertices.shape[0], 6, 32, 32, 0, 6
    d.cos_thresh, d.two_sqrt3 = float(np.float32(math.cos(math.radians(100.0)))), float(np.float32(2.0 * math.sqrt(3.0)))
    assert lib.utx_backproject_vis(h, C.byref(d), None, 0, s["bvh"].handle, st) == -2      # no alpha plane
    d.images = ptr(s["alpha"])
    assert lib.utx_backproject_vis(h, C.byref(d), None, 2, s["bvh"].handle, st) == -2      # no such sample mode
    d.view_count = 7
    assert lib.utx_backproject_vis(h, C.byref(d), None, 0, s["bvh"].handle, st) == -2      # views beyond n_views
    d.view_count = 6
    assert lib.utx_backproject_vis(h, C.byref(d), None, 0, s["bvh"].handle, st) == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="utx_lens_blur_seam_c"):
        ops.lens_blur_seam(torch.zeros(Hh, Ww, 17, device="cuda"), seam)
