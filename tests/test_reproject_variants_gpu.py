"""Back-projection variants on the GPU: reproject_method='gaussian', the seam window sizes and grid_interpolate_mode='nvdiff' through
NVDiffRendererInverse.infer against the reference's own outputs (fixtures G67g / G67n, tests/golden/make_golden_reproject_variants.py), and the three
new entry points (utx_seam_mask_sized, utx_gaussian_blur_seam, utx_backproject_sampled) against the numpy restatements of
oracle/reproject_ref.py and the oracle, at scale, on all three traversal modes, and under view sharding."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from oracle import geom_ref as G
from oracle import reproject_ref as RV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _infer(f, images, alpha, c2ws, intr, **kw):
    """infer() on a G67-style fixture; the view alpha the generator holed is substituted at the mv_to_pcd seam, as in G67 / G67p"""
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    n, HW = images.shape[:2]
    seen = {}

    class Inv(NVDiffRendererInverse):
        def mv_to_pcd(self, *a, **k):
            out = super().mv_to_pcd(*a, **k)
            seen["mv_alpha"] = out["alpha"].clone()
            out["alpha"] = torch.from_numpy(alpha).to(out["alpha"].device).contiguous()
            return out
    inv = Inv(device="cuda").update_from_arrays(f["verts"], f["faces"], f["uvs"])
    out = inv.infer(None, c2ws=c2ws, intrinsics=intr, image_attrs=torch.from_numpy(images), H=HW, W=HW, H2D=96, W2D=96,
                    ray_normal_angle_threhold=100.0, method="reproject", filt_gradient_points=False, return_layers=True, **kw)
    torch.cuda.synchronize()
    return inv, out, seen


def _check_atlas(name, got, ref):
    err = np.abs(got - ref)
    print("%s final atlas: max |d| %.3g, median %.3g, share beyond 1e-4: %.5f" % (name, err.max(), np.median(err), (err > 1e-4).mean()))
    assert (err > 1e-4).mean() < 2e-3 and np.median(err) < 1e-6


@pytest.mark.parametrize("tag,sizes", [("d", (3, 3, 5)), ("s", (5, 5, 7))])
def test_g67g_gaussian_fixture_through_infer(tag, sizes):
    """infer(reproject_method='gaussian', reproject_kernel_size_*) on G67g, with the bounds of test_g67p_perspective_backprojection_fixture_through_infer;
    the seam equals the numpy restatement of the generalised identity on the run's own winner map"""
    f = RV.load("g67g_reproject_gaussian.npz")
    imgs = f["images"].astype(F32)
    n, HW, T = 6, imgs.shape[1], 96
    alpha = RV.unpack(f["alpha"], (n, HW, HW, 1))[..., 0].astype(F32)
    kb, kbb, kblur = sizes
    inv, (textured, mask_vis, mask_2d, color_2d, layers, vis), seen = _infer(
        f, imgs, alpha, f["c2ws"], f["intr"], perspective=True, reproject_method="gaussian", reproject_kernel_size_boundary=kb,
        reproject_kernel_size_boundary_blur=kbb, reproject_kernel_size_blur=kblur)
    assert np.array_equal(seen["mv_alpha"].cpu().numpy().astype(bool), RV.unpack(f["mv_alpha"], (n, HW, HW, 1))[..., 0])
    cov = mask_2d.cpu().numpy()[0, ..., 0]
    assert np.array_equal(cov, RV.unpack(f["mask_2d"], (1, T, T, 1))[0, ..., 0])
    got_vis, ref_vis = mask_vis.cpu().numpy()[..., 0], RV.unpack(f["mask_2d_visiable"], (n, T, T, 1))[..., 0]
    mism = int((got_vis != ref_vis).sum())
    print("G67g %s visibility: %d of %d texel-views differ" % (tag, mism, ref_vis.size))
    assert mism <= 2
    win = inv.last["winner"].cpu().numpy().astype(np.int32)
    seam = inv.last["seam"].cpu().numpy().astype(bool)
    assert np.array_equal(seam, RV.seam_identity(win, cov, kb, kbb)), "seam mask at (%d, %d)" % (kb, kbb)
    _check_atlas("G67g " + tag, color_2d.cpu().numpy()[0], f["color_2d_gauss_" + tag][0])
    if tag == "s":
        pre = inv.last["atlas_prefill"].cpu().numpy()[cov]
        err = np.abs(pre - f["pre_gauss_s"])
        print("G67g s blurred atlas before pull-push: max |d| %.3g, share beyond 1e-4 %.5f" % (err.max(), (err > 1e-4).mean()))
        assert (err > 1e-4).mean() < 2e-3 and np.median(err) < 1e-6
    # the lens run on the same inputs blurs the same seam another way
    _, lens, _ = _infer(f, imgs, alpha, f["c2ws"], f["intr"], perspective=True, reproject_kernel_size_boundary=kb, reproject_kernel_size_boundary_blur=kbb)
    assert not torch.equal(lens[3], color_2d)


@pytest.mark.parametrize("tag", ["o", "p"])
def test_g67n_nvdiff_fixture_through_infer(tag):
    f = RV.load("g67n_backprojection_nvdiff.npz")
    imgs = f["images"].astype(F32)
    n, HW, T = 6, imgs.shape[1], 96
    alpha = RV.unpack(f["alpha_" + tag], (n, HW, HW, 1))[..., 0].astype(F32)
    persp = tag == "p"
    inv, (textured, mask_vis, mask_2d, color_2d, layers, vis), seen = _infer(f, imgs, alpha, f["c2ws_" + tag], f["intr_" + tag], perspective=persp,
                                                                             grid_interpolate_mode="nvdiff")
    assert np.array_equal(seen["mv_alpha"].cpu().numpy().astype(bool), RV.unpack(f["mv_alpha_" + tag], (n, HW, HW, 1))[..., 0])
    got_vis, ref_vis = mask_vis.cpu().numpy()[..., 0], RV.unpack(f["mask_2d_visiable_" + tag], (n, T, T, 1))[..., 0]
    mism = int((got_vis != ref_vis).sum())
    print("G67n %s visibility: %d of %d texel-views differ" % (tag, mism, ref_vis.size))
    assert mism <= 2
    if persp:
        both = got_vis & ref_vis
        ref_cols = np.zeros((n, T, T, 3), F32)
        ref_cols[ref_vis] = f["vis_colors_p"]
        assert np.abs(ref_cols[both] - layers.cpu().numpy()[both]).max() < 2e-6, "per-view wrap-sampled colours"
    _check_atlas("G67n " + tag, color_2d.cpu().numpy()[0], f["color_2d_" + tag][0])
    # 'nvdiffrast' is the same mode; 'torch' is the zero-padded one, as in the reference's own 'torch' run
    _, alias, _ = _infer(f, imgs, alpha, f["c2ws_" + tag], f["intr_" + tag], perspective=persp, grid_interpolate_mode="nvdiffrast")
    assert torch.equal(alias[3], color_2d) and torch.equal(alias[1], mask_vis)
    _, grid, _ = _infer(f, imgs, alpha, f["c2ws_" + tag], f["intr_" + tag], perspective=persp)
    ref_t = RV.unpack(f["mask_2d_visiable_torch_" + tag], (n, T, T, 1))[..., 0]
    assert int((grid[1].cpu().numpy()[..., 0] != ref_t).sum()) <= 2
    assert int((grid[1] != mask_vis).sum()) >= 20


def _seam_sized(winner, rast2d, kb, kbb):
    """utx_seam_mask_sized called directly (ops.seam_mask takes utx_seam_mask at 3 / 3)"""
    from unitex_amd._lib import ptr
    from unitex_amd.flux.ops import get_ctx
    ctx = get_ctx(winner.device.index)
    H, W = winner.shape
    tmp = torch.empty(4, H, W, dtype=torch.uint8, device=winner.device)
    seam = torch.empty(H, W, dtype=torch.uint8, device=winner.device)
    ctx.check(ctx.lib.utx_seam_mask_sized(ctx.handle, ptr(winner), ptr(rast2d), H, W, kb, kbb, ptr(tmp), ptr(seam), ctx.stream()))
    return seam


def test_seam_mask_sized_at_3_3_is_bit_identical_to_the_default():
    from unitex_amd.texturetools import ops
    f = RV.load("g67_backprojection.npz")
    vis = f["mask_2d_visiable"][..., 0].astype(bool)
    cov = f["mask_2d"][0, ..., 0].astype(bool)
    rast = np.zeros(cov.shape + (4,), F32)
    rast[..., 3] = cov
    cases = [(torch.from_numpy(RV.winner_of(vis).astype(np.int8)), torch.from_numpy(rast))]
    cases += [RV._blob_winner(2048, 2048, s, 400) for s in (1, 2)]
    for w, r in cases:
        w, r = w.cuda().contiguous(), r.cuda().contiguous()
        default = ops.seam_mask(w, r)
        assert torch.equal(_seam_sized(w, r, 3, 3), default)
        assert torch.equal(_seam_sized(w, r, 2, 2), default)       # the windows are 2 (k // 2) + 1 wide
        assert int(default.sum()) > 100


@pytest.mark.parametrize("H,W,seed", [(37, 53, 3), (257, 300, 4), (1024, 768, 5)])
def test_seam_mask_sized_equals_the_numpy_identity(H, W, seed):
    from unitex_amd.texturetools import ops
    w, r = RV._blob_winner(H, W, seed, 60)
    wd, rd = w.cuda().contiguous(), r.cuda().contiguous()
    cov = r[..., 3].numpy() > 0
    for kb, kbb in [(5, 5), (0, 3), (3, 0), (1, 7), (9, 4), (17, 2), (31, 31), (30, 31)]:
        ref = RV.seam_identity(w.numpy(), cov, kb, kbb)
        got = ops.seam_mask(wd, rd, kb, kbb).cpu().numpy().astype(bool)
        assert np.array_equal(got, ref), "seam (%d, %d) at %d x %d" % (kb, kbb, H, W)
        if (kb, kbb) == (5, 5):
            assert ref.any() and not ref.all()


def _gauss_ref_at(src, k, ys, xs):
    """the fp64 reference (RV.gaussian_blur_fp64) at a list of texels: w1[i] * w1[j] in fp32, reflect padding"""
    w1 = RV.gaussian_w1(k)
    w2 = (w1[:, None] * w1[None, :]).astype(F32).astype(np.float64)
    H, W = src.shape[:2]
    r = k // 2
    refl = lambda i, n: np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
    out = np.zeros((len(ys), 3), np.float64)
    for i in range(k):
        yy = refl(ys + i - r, H)
        for j in range(k):
            out += w2[i, j] * src[yy, refl(xs + j - r, W)].astype(np.float64)
    return out


@pytest.mark.parametrize("k", [1, 3, 5, 7, 31])
def test_gaussian_blur_seam_within_1e6_of_fp64(k):
    from unitex_amd.texturetools import ops
    g = torch.Generator().manual_seed(k)
    # 2048^2, a sparse seam that touches all four borders (checked at a sample of seam texels; the rest must be src bit for bit)
    H = W = 2048
    src = torch.rand(H, W, 3, generator=g)
    seam = (torch.rand(H, W, generator=g) < 0.02)
    seam[0, :] = seam[-1, :] = True
    seam[:, 0] = seam[:, -1] = True
    out = ops.gaussian_blur_seam(src.cuda(), seam.to(torch.uint8).cuda(), k).cpu().numpy()
    s, sm = src.numpy(), seam.numpy()
    assert np.array_equal(out[~sm], s[~sm])
    ys, xs = np.nonzero(sm)
    pick = np.random.default_rng(k).choice(len(ys), 20000, replace=False)
    pick = np.concatenate([pick, np.nonzero((ys == 0) | (xs == W - 1))[0][:4000]])
    ref = _gauss_ref_at(s, k, ys[pick], xs[pick])
    assert np.abs(out[ys[pick], xs[pick]] - ref).max() <= 1e-6
    # small odd sizes with the whole image as seam: every texel against the fp64 conv
    for h, w in ((33, 17), (k // 2 + 1, k // 2 + 2), (41, 39)):
        src = torch.rand(h, w, 3, generator=g)
        seam = torch.ones(h, w, dtype=torch.uint8)
        out = ops.gaussian_blur_seam(src.cuda(), seam.cuda(), k).cpu().numpy()
        assert np.abs(out - RV.gaussian_blur_fp64(src.numpy(), k)).max() <= 1e-6, "%d x %d, k %d" % (h, w, k)


def _wrap_scene(n_faces, persp):
    """six views of a sphere that crosses every view border (fov 49.1 at radius 1.8, or orthographic with the unit sphere at ndc +-1.15), 512^2
    views with alpha = coverage, a 1024^2 atlas"""
    from unitex_amd.texturetools import camera, ops
    from unitex_amd.texturetools.benchmarks import smooth_views
    from unitex_amd.texturetools.meshes import sphere_with_faces
    verts, faces, uvs = sphere_with_faces(n_faces)
    T, HW, n = 1024, 512, 6
    if persp:
        c2ws = camera.generate_box_views_c2ws(1.8)[[0, 1, 4, 2, 3, 5]]
        intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    else:
        c2ws = camera.generate_box_views_c2ws(2.8)[[0, 1, 4, 2, 3, 5]]
        intr = camera.generate_intrinsics(1.15, 1.15, fov=False, degree=False)
    mvp = torch.matmul(camera.intr_to_proj(intr, perspective=persp), camera.c2w_to_w2c(c2ws))
    vd, fd = _cu(verts), _cu(faces)
    clip, ndc = ops.transform_points(vd, mvp.cuda().contiguous())
    uvclip = np.concatenate([uvs * 2 - 1, np.zeros((len(uvs), 1), F32), np.ones((len(uvs), 1), F32)], -1)
    rast_d = ops.rasterize(_cu(uvclip), fd, T, T)
    imgs = np.zeros((n, HW, HW, 4), F32)
    imgs[..., :3] = smooth_views(n, HW, HW)
    for v in range(n):
        imgs[v, ..., 3] = (ops.rasterize(clip[v].contiguous(), fd, HW, HW)[..., 3] > 0).float().cpu().numpy()
    return dict(verts=verts, faces=faces, vd=vd, fd=fd, ndc=ndc.contiguous(), rast_d=rast_d, imgs=imgs, fn=G.face_normals(verts, faces),
                eyes=np.ascontiguousarray(c2ws[:, :3, 3].numpy(), F32), dirs=(-c2ws[:, :3, 2]).numpy().astype(F32))


@pytest.mark.parametrize("n_faces", [20000, 50000])
@pytest.mark.parametrize("persp", [False, True])
def test_nvdiff_sampling_bit_exact_at_scale(n_faces, persp):
    """utx_backproject_sampled(sample_mode=1): colour and alpha against the numpy wrap sampling at the oracle's NDC interpolation, ray visibility
    against the oracle's LBVH walk, on the packet walk (default), the stackless thread walk and the stack walk; rayvis equals the grid mode's,
    and sample_mode=0 equals utx_backproject / utx_backproject_persp"""
    from unitex_amd import _lib
    from unitex_amd.texturetools import ops
    s = _wrap_scene(n_faces, persp)
    rast2d = s["rast_d"].cpu().numpy()
    bvh_ref = G.BVH(s["verts"], s["faces"])
    col_g, rv_ref, ao_g = G.backproject(rast2d, s["verts"], s["faces"], s["fn"], s["ndc"].cpu().numpy(), s["dirs"], s["imgs"], bvh_ref, angle_deg=115.0)
    if persp:
        rv_ref = RV.texel_rayvis(rast2d, s["verts"], s["faces"], s["fn"], s["eyes"], bvh_ref, 115.0)
    col_ref, ao_ref = RV.backproject_nvdiff(rast2d, s["verts"], s["faces"], s["fn"], s["ndc"].cpu().numpy(), s["imgs"], rv_ref)
    assert int((ao_ref != ao_g).sum()) > 100, "the wrap must change the alpha test along the view borders"
    bvh = ops.BVH(s["vd"], s["fd"])
    eyes = _cu(s["eyes"]) if persp else None
    dirs = None if persp else _cu(s["dirs"])
    args = (s["rast_d"], s["vd"], s["fd"], _cu(s["fn"]), s["ndc"], dirs, _cu(s["imgs"]), bvh)
    assert _lib.get_options()["UTX_BVH_PACKET"] == 1 and _lib.get_options()["UTX_BVH_STACK_WALK"] == 0
    try:
        for packet, stack in ((1, 0), (0, 0), (0, 1)):
            _lib.set_option("UTX_BVH_PACKET", packet); _lib.set_option("UTX_BVH_STACK_WALK", stack)
            col, rv, ao = ops.backproject(*args, angle_deg=115.0, eyes=eyes, sample="nvdiff")
            assert np.array_equal(rv.cpu().numpy(), rv_ref), "ray visibility (packet %d, stack walk %d)" % (packet, stack)
            assert np.array_equal(ao.cpu().numpy(), ao_ref), "wrap-sampled alpha mask"
            assert np.array_equal(col.cpu().numpy(), col_ref), "wrap-sampled colours"
            col0, rv0, ao0 = ops.backproject(*args, angle_deg=115.0, eyes=eyes)
            assert torch.equal(rv0, rv), "rayvis does not depend on the sampling"
            # sample_mode=0 through the new entry point is the existing launch
            c1, r1, a1 = (torch.zeros_like(col0), torch.zeros_like(rv0), torch.zeros_like(ao0))
            _sampled(args, eyes, 0, (c1, r1, a1))
            assert torch.equal(c1, col0) and torch.equal(r1, rv0) and torch.equal(a1, ao0)
    finally:
        _lib.set_option("UTX_BVH_PACKET", 1); _lib.set_option("UTX_BVH_STACK_WALK", 0)
    # the grid mode's colour and alpha do not depend on the rays: the oracle's zero-padded gather
    assert np.array_equal(ao0.cpu().numpy(), ao_g) and np.array_equal(col0.cpu().numpy(), col_g)
    assert 0.05 < rv_ref.mean() < 0.9


def _sampled(args, eyes, mode, out):
    """utx_backproject_sampled with the descriptor ops.backproject builds"""
    import math
    from unitex_amd._lib import BackprojectDesc, ptr
    from unitex_amd.flux.ops import get_ctx
    rast2d, verts, faces, fnormal, vndc, dirs, images, bvh = args
    ctx = get_ctx(rast2d.device.index)
    Th, Tw = rast2d.shape[:2]
    n, H, W = images.shape[:3]
    d = BackprojectDesc()
    d.rast2d, d.verts, d.faces, d.fnormal, d.vndc, d.images = ptr(rast2d), ptr(verts), ptr(faces), ptr(fnormal), ptr(vndc), ptr(images)
    if dirs is not None:
        d.dirs = ptr(dirs)
    d.color, d.rayvis, d.alphaok = ptr(out[0]), ptr(out[1]), ptr(out[2])
    d.T_h, d.T_w, d.V, d.n_views, d.H, d.W = Th, Tw, verts.shape[0], n, H, W
    d.view_begin, d.view_count = 0, n
    d.cos_thresh = float(np.float32(math.cos(math.radians(115.0))))
    d.two_sqrt3 = float(np.float32(2.0 * math.sqrt(3.0)))
    rc = ctx.lib.utx_backproject_sampled(ctx.handle, C.byref(d), None if eyes is None else ptr(eyes), mode, bvh.handle, ctx.stream())
    ctx.check(rc)


def _sharded_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from unitex_amd.texturetools import camera, meshes
        from unitex_amd.texturetools.benchmarks import smooth_views
        from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
        dev = "cuda:0"
        torch.cuda.set_device(0)
        verts, faces, uvs = meshes.sphere_with_faces(20000)
        c2ws = camera.generate_box_views_c2ws(1.8)[[0, 1, 4, 2, 3, 5]]
        intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
        images = torch.from_numpy(smooth_views(6, 256, 256)).to(dev)
        kw = dict(c2ws=c2ws, intrinsics=intr, image_attrs=images, perspective=True, H=256, W=256, H2D=512, W2D=512,
                  filt_gradient_points=True, ray_normal_angle_threhold=115.0, return_layers=True, grid_interpolate_mode="nvdiff",
                  reproject_method="gaussian", reproject_kernel_size_boundary=5, reproject_kernel_size_blur=7)
        inv = NVDiffRendererInverse(device=dev, view_shard=(rank, world)).update_from_arrays(verts, faces, uvs)
        out = inv.infer(None, **kw)
        torch.cuda.synchronize()
        res = {"rank": rank}
        if rank == 0:
            one = NVDiffRendererInverse(device=dev).update_from_arrays(verts, faces, uvs)
            ref = one.infer(None, **kw)
            torch.cuda.synchronize()
            res["texture_equal"] = bool(np.array_equal(out[0].texture, ref[0].texture))
            res["color2d_equal"] = bool(torch.equal(out[3], ref[3]))
            res["vis_equal"] = bool(torch.equal(out[1], ref[1]))
            res["layers_equal"] = bool(torch.equal(out[4], ref[4]) and torch.equal(out[5], ref[5]))
            res["seam_equal"] = bool(torch.equal(inv.last["seam"], one.last["seam"]))
            res["seam"] = float(one.last["seam"].float().mean())
            grid = NVDiffRendererInverse(device=dev).update_from_arrays(verts, faces, uvs).infer(None, **dict(kw, grid_interpolate_mode="torch"))
            torch.cuda.synchronize()
            res["differs_from_grid"] = not torch.equal(grid[1], ref[1])
        dist.barrier()
        if rank == 0:
            q.put(res)
    finally:
        dist.destroy_process_group()


def test_view_sharded_nvdiff_gaussian_infer_is_bit_identical_to_one_rank():
    """two gloo ranks on one GPU, each back-projecting three views with the nvdiff sampling, then the Gaussian seam blur at 5 / 3 / 7"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29950 + (os.getpid() % 30)
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res["seam"] > 0.001 and res["differs_from_grid"]
    for k, v in res.items():
        if k.endswith("_equal"):
            assert v, "%s differs between world=2 and world=1: %s" % (k, res)


def test_bad_arguments_fail_as_the_reference_does():
    from unitex_amd.texturetools import ops
    f = RV.load("g67g_reproject_gaussian.npz")
    imgs = f["images"].astype(F32)
    alpha = RV.unpack(f["alpha"], (6, 48, 48, 1))[..., 0].astype(F32)
    bad = [(AssertionError, dict(reproject_method="box")), (AssertionError, dict(grid_interpolate_mode="cuda")),
           (ValueError, dict(reproject_method="gaussian", reproject_kernel_size_blur=4)),
           (ValueError, dict(reproject_method="gaussian", reproject_kernel_size_blur=0)),
           (ValueError, dict(reproject_method="gaussian", reproject_kernel_size_blur=-3)),
           (NotImplementedError, dict(reproject_method="gaussian", reproject_kernel_size_blur=33)),
           (NotImplementedError, dict(reproject_kernel_size_boundary=32)),
           (NotImplementedError, dict(reproject_kernel_size_boundary_blur=33)),
           (ValueError, dict(reproject_kernel_size_boundary=-1)),
           (NotImplementedError, dict(return_mv_reproject_uv=True)), (TypeError, dict(reproject_kernel_size=3))]
    for exc, kw in bad:
        with pytest.raises(exc) as e:
            _infer(f, imgs, alpha, f["c2ws"], f["intr"], perspective=True, **kw)
        if exc is NotImplementedError and "reproject_kernel_size" in str(kw):
            assert ("31" in str(e.value)) or ("15" in str(e.value)), "the cap is named in the message"
    # the lens blur ignores reproject_kernel_size_blur, as the reference does; 31 is the largest size built
    _infer(f, imgs, alpha, f["c2ws"], f["intr"], perspective=True, reproject_kernel_size_blur=4)
    _infer(f, imgs, alpha, f["c2ws"], f["intr"], perspective=True, reproject_method="gaussian", reproject_kernel_size_blur=31,
           reproject_kernel_size_boundary=31, reproject_kernel_size_boundary_blur=31)
    # the C entry points refuse out-of-range sizes and modes with -2
    w = torch.zeros(16, 16, dtype=torch.int8, device="cuda")
    r = torch.zeros(16, 16, 4, device="cuda")
    with pytest.raises(RuntimeError, match="utx_seam_mask_sized"):
        _seam_sized(w, r, 32, 3)
    with pytest.raises(RuntimeError, match="utx_seam_mask_sized"):
        _seam_sized(w, r, 3, -1)
    src = torch.rand(16, 16, 3, device="cuda")
    seam = torch.ones(16, 16, dtype=torch.uint8, device="cuda")
    for k in (4, 33):
        with pytest.raises(RuntimeError, match="utx_gaussian_blur_seam"):
            ops.gaussian_blur_seam(src, seam, k)
    with pytest.raises(RuntimeError, match="utx_gaussian_blur_seam"):      # k // 2 must stay below min(H, W) (reflect padding)
        ops.gaussian_blur_seam(src[:4].contiguous(), seam[:4].contiguous(), 9)
    s = _wrap_scene(2000, False)
    args = (s["rast_d"], s["vd"], s["fd"], _cu(s["fn"]), s["ndc"], _cu(s["dirs"]), _cu(s["imgs"]), ops.BVH(s["vd"], s["fd"]))
    n, T = 6, s["rast_d"].shape[0]
    out = (torch.zeros(n, T, T, 3, device="cuda"), torch.zeros(n, T, T, dtype=torch.uint8, device="cuda"), torch.zeros(n, T, T, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="utx_backproject_sampled"):
        _sampled(args, None, 2, out)
    with pytest.raises(RuntimeError, match="utx_backproject_sampled"):
        _sampled(args[:5] + (None,) + args[6:], None, 1, out)       # orthographic without directions
