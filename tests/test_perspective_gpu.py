"""Perspective cameras on the GPU: utx_backproject_persp / utx_view_visibility_persp through NVDiffRendererInverse.infer and
VideoExporter.export_condition against the reference's own outputs (fixtures G67p, G11p, G9p: tests/golden/make_golden_perspective.py), and
bit for bit against the oracle + the numpy restatement of the perspective rays (oracle/reproject_ref.py) at scale, on all three
traversal modes, and under view sharding."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import geom_ref as G
from oracle import reproject_ref as PC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _g67p_infer(f, **kw):
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    imgs = f["images"].astype(F32)
    n, HW = imgs.shape[:2]
    alpha = PC.unpack(f["alpha"], (n, HW, HW, 1))[..., 0].astype(F32)
    seen = {}

    class Inv(NVDiffRendererInverse):
        def mv_to_pcd(self, *a, **k):      # the fixture's view alpha is holed by the generator: substituted at this one seam, as in G6/G7
            out = super().mv_to_pcd(*a, **k)
            seen["mv_alpha"] = out["alpha"].clone()
            out["alpha"] = torch.from_numpy(alpha).to(out["alpha"].device).contiguous()
            return out
    inv = Inv(device="cuda").update_from_arrays(f["verts"], f["faces"], f["uvs"])
    out = inv.infer(None, c2ws=f["c2ws"], intrinsics=f["intr"], image_attrs=torch.from_numpy(imgs), H=HW, W=HW, H2D=96, W2D=96,
                    ray_normal_angle_threhold=100.0, method="reproject", filt_gradient_points=False, return_layers=True, **kw)
    torch.cuda.synchronize()
    return inv, out, seen


def test_g67p_perspective_backprojection_fixture_through_infer():
    """infer(perspective=True, method='reproject') on G67p, with the checks and bounds of test_g67_backprojection_fixture_through_infer"""
    from unitex_amd.texturetools.renderer_inverse import PRIORITY
    f = PC.load("g67p_backprojection_perspective.npz")
    n, HW, T = 6, f["images"].shape[1], 96
    inv, (textured, mask_vis, mask_2d, color_2d, layers, vis), seen = _g67p_infer(f, perspective=True)
    assert np.array_equal(seen["mv_alpha"].cpu().numpy().astype(bool), PC.unpack(f["mv_alpha"], (n, HW, HW, 1))[..., 0]), "perspective view coverage"
    assert np.array_equal(mask_2d.cpu().numpy()[0, ..., 0], PC.unpack(f["mask_2d"], (1, T, T, 1))[0, ..., 0]), "atlas coverage"
    got_vis, ref_vis = mask_vis.cpu().numpy()[..., 0], PC.unpack(f["mask_2d_visiable"], (n, T, T, 1))[..., 0]
    mism = int((got_vis != ref_vis).sum())
    print("G67p visibility: %d of %d texel-views differ" % (mism, ref_vis.size))
    assert mism <= 2
    both = got_vis & ref_vis
    ref_cols = np.zeros((n, T, T, 3), F32)
    ref_cols[ref_vis] = f["vis_colors"]
    assert np.abs(ref_cols[both] - layers.cpu().numpy()[both]).max() < 2e-6, "per-view gathered colours"
    agree = (got_vis == ref_vis).all(0)
    exp = np.full((T, T), -1, np.int32)
    for v in reversed(PRIORITY):
        exp[ref_vis[v]] = v
    win = inv.last["winner"].cpu().numpy().astype(np.int32)
    assert np.array_equal(win[agree], exp[agree]), "composite winner index"
    assert ((win < 0) & mask_2d.cpu().numpy()[0, ..., 0]).sum() > 50, "the case must have unseen texels"
    err = np.abs(color_2d.cpu().numpy()[0] - f["color_2d"][0])
    print("G67p final atlas: max |d| %.3g, median %.3g, share beyond 1e-4: %.5f" % (err.max(), np.median(err), (err > 1e-4).mean()))
    assert (err > 1e-4).mean() < 2e-3 and np.median(err) < 1e-6
    assert textured.texture.shape == (T, T, 3)


def test_infer_runs_with_the_reference_default_perspective():
    """infer() without a `perspective` keyword takes the reference's default (perspective=True) instead of stopping at an assert"""
    f = PC.load("g67p_backprojection_perspective.npz")
    _, default, _ = _g67p_infer(f)
    _, explicit, _ = _g67p_infer(f, perspective=True)
    assert torch.equal(default[3], explicit[3]) and torch.equal(default[1], explicit[1])
    _, ortho, _ = _g67p_infer(f, perspective=False)
    assert not torch.equal(ortho[1], explicit[1])


def test_g11p_perspective_gradient_filter_and_order_mean_bake():
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    f = PC.load("g11p_filter_and_kdtree_perspective.npz")
    imgs = torch.from_numpy(f["images"].astype(F32))
    n, HW, T = 6, 96, 96
    inv = NVDiffRendererInverse(device="cuda").update_from_arrays(f["verts"], f["faces"], f["uvs"])
    out = inv.infer(None, c2ws=torch.from_numpy(f["c2ws"]), intrinsics=torch.from_numpy(f["intr"]), image_attrs=imgs, perspective=True,
                    H=HW, W=HW, H2D=T, W2D=T, method="kdtree", grad_norm_threhold=0.20, ray_normal_angle_threhold=115.0,
                    filt_gradient_points=True, kdtree_method="order_mean", kdtree_n_neighbors_visiable=1, kdtree_n_neighbors_invisiable=4)
    torch.cuda.synchronize()
    ref_vis = PC.unpack(f["mask_visiable"], (n, HW, HW, 1))[..., 0]
    mism = int((inv.last["view_mask"].cpu().numpy().astype(bool) != ref_vis).sum())
    print("G11p view masks: %d differ" % mism)
    assert mism <= 8, "filtered view masks vs the reference"
    ref_v2d = PC.unpack(f["mask_2d_visiable"], (n, T, T, 1))[..., 0]
    assert int((out[1][..., 0].cpu().numpy() != ref_v2d).sum()) <= 24, "texel visibility vs the reference"
    err = np.abs(out[3][0].cpu().numpy() - f["color_2d_order_mean"][0])
    print("G11p order_mean atlas: max %.3g, median %.3g, share beyond 1e-3 %.5f" % (err.max(), np.median(err), (err > 1e-3).mean()))
    assert (err > 1e-3).mean() < 2e-2 and np.median(err) < 1e-6


def test_view_visibility_perspective_bit_exact():
    """utx_view_visibility_persp against the numpy restatement, on the G11p scene's interpolated attributes, at three thresholds"""
    from unitex_amd.texturetools import ops
    f = PC.load("g11p_filter_and_kdtree_perspective.npz")
    s = PC.scene(f)
    n, HW = 6, 96
    va = np.concatenate([s["verts"], G.vertex_normals_area(s["verts"], s["faces"])], -1).astype(F32)
    rast = np.stack([G.rasterize(s["clip"][v], s["faces"], HW, HW) for v in range(n)])
    attr = np.stack([G.interpolate(va, rast[v], s["faces"]) for v in range(n)])
    for thr, ang in ((0.20, 115.0), (0.15, 100.0), (0.5, 95.0)):
        ref = PC.view_visibility_persp(attr, rast, s["fn"], s["eyes"], grad_thr=thr, angle_deg=ang)
        vis, alpha = ops.view_visibility(_cu(attr), _cu(rast), _cu(s["fn"]), None, grad_thr=thr, angle_deg=ang, eyes=_cu(s["eyes"]))
        assert np.array_equal(vis.cpu().numpy().astype(bool), ref), "perspective view mask (thr %g, angle %g)" % (thr, ang)
        assert np.array_equal(alpha.cpu().numpy(), ref.astype(F32))
        assert 0.02 < ref.mean() < 0.9


@pytest.mark.parametrize("n_faces", [20000, 50000])
def test_perspective_backprojection_bit_exact_at_scale(n_faces):
    """six 512^2 perspective views (fov 49.1, box cameras at 2.8) into a 1024^2 atlas: colour and alpha (ray-independent) against the oracle's
    gather at the perspective NDC, ray visibility against the oracle's LBVH walk of the numpy perspective rays, the hole-filled visibility
    against the oracle's dilation -- bit for bit, on the packet walk (default), the stackless thread walk and the stack walk"""
    from unitex_amd import _lib
    from unitex_amd.texturetools import camera, ops
    from unitex_amd.texturetools.benchmarks import smooth_views
    from unitex_amd.texturetools.meshes import sphere_with_faces
    verts, faces, uvs = sphere_with_faces(n_faces)
    T, HW, n = 1024, 512, 6
    c2ws = camera.generate_box_views_c2ws(2.8)[[0, 1, 4, 2, 3, 5]]
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    mvp = torch.matmul(camera.intr_to_proj(intr, perspective=True), camera.c2w_to_w2c(c2ws))
    vd, fd = _cu(verts), _cu(faces)
    clip, ndc = ops.transform_points(vd, mvp.cuda().contiguous())
    uvclip = np.concatenate([uvs * 2 - 1, np.zeros((len(uvs), 1), F32), np.ones((len(uvs), 1), F32)], -1)
    rast_d = ops.rasterize(_cu(uvclip), fd, T, T)
    rast2d = rast_d.cpu().numpy()
    imgs = np.zeros((n, HW, HW, 4), F32)
    imgs[..., :3] = smooth_views(n, HW, HW)
    for v in range(n):
        imgs[v, ..., 3] = (ops.rasterize(clip[v].contiguous(), fd, HW, HW)[..., 3] > 0).float().cpu().numpy()
    fn = G.face_normals(verts, faces)
    eyes = np.ascontiguousarray(c2ws[:, :3, 3].numpy(), F32)
    dirs = (-c2ws[:, :3, 2]).numpy().astype(F32)
    bvh_ref = G.BVH(verts, faces)
    col_ref, _, ao_ref = G.backproject(rast2d, verts, faces, fn, ndc.cpu().numpy(), dirs, imgs, bvh_ref, angle_deg=115.0)
    rv_ref = PC.texel_rayvis(rast2d, verts, faces, fn, eyes, bvh_ref, 115.0)
    vis_ref = G.dilate_visibility(rv_ref, rast2d[..., 3] > 0, ao_ref)
    bvh = ops.BVH(vd, fd)
    args = (rast_d, vd, fd, _cu(fn), ndc.contiguous(), None, _cu(imgs), bvh)
    assert _lib.get_options()["UTX_BVH_PACKET"] == 1 and _lib.get_options()["UTX_BVH_STACK_WALK"] == 0
    try:
        for packet, stack in ((1, 0), (0, 0), (0, 1)):
            _lib.set_option("UTX_BVH_PACKET", packet); _lib.set_option("UTX_BVH_STACK_WALK", stack)
            col, rv, ao = ops.backproject(*args, angle_deg=115.0, eyes=_cu(eyes))
            assert np.array_equal(rv.cpu().numpy(), rv_ref), "perspective ray visibility (packet %d, stack walk %d)" % (packet, stack)
            assert np.array_equal(ao.cpu().numpy(), ao_ref), "alpha mask"
            assert np.array_equal(col.cpu().numpy(), col_ref), "gathered colours"
            vis = ops.dilate_visibility(rv, ao, rast_d)
            assert np.array_equal(vis.cpu().numpy().astype(bool), vis_ref), "hole-filled visibility"
    finally:
        _lib.set_option("UTX_BVH_PACKET", 1); _lib.set_option("UTX_BVH_STACK_WALK", 0)
    assert 0.05 < rv_ref.mean() < 0.9
    # the orthographic launch on the same inputs is another ray model: it must not coincide
    _, rv_o, _ = ops.backproject(rast_d, vd, fd, _cu(fn), ndc.contiguous(), _cu(dirs), _cu(imgs), bvh, angle_deg=115.0)
    assert not np.array_equal(rv_o.cpu().numpy(), rv_ref)


def test_g9p_orbit_perspective_condition_render_matches_reference():
    """export_condition(orbit=True, perspective=True, 4 views, 2 x 2) against the reference's own run, with the bounds of
    test_condition_render_matches_reference_fixture"""
    from unitex_amd.texturetools.video import VideoExporter
    f = PC.load("g9p_export_condition_perspective.npz")
    out = VideoExporter(device="cuda:0", normal_weighting="area").export_condition((f["verts"], f["faces"]), geometry_scale=0.95, n_views=4, n_rows=2,
                                                                                  n_cols=2, H=64, W=64, fov_deg=49.1, scale=1.0, perspective=True,
                                                                                  orbit=True, background="grey", return_image=True, return_camera=True)
    assert np.array_equal(np.asarray(out["alpha"]), f["alpha"])
    for key in ("ccm", "normal"):
        d = np.abs(np.asarray(out[key]).astype(np.int32) - f[key].astype(np.int32))
        print("G9p %s: max %d, share differing %.5f" % (key, int(d.max()), float((d > 0).mean())))
        assert d.max() <= 1, "%s differs by %d" % (key, int(d.max()))
        assert (d > 0).mean() < 5e-3, "%s: %.4f of the bytes differ" % (key, float((d > 0).mean()))
    assert np.array_equal(out["c2ws"].numpy(), f["c2ws"]) and np.array_equal(out["intrinsics"].numpy(), f["intrinsics"])
    assert out["perspective"] is True


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
        c2ws = camera.generate_box_views_c2ws(2.8)[[0, 1, 4, 2, 3, 5]]
        intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
        images = torch.from_numpy(smooth_views(6, 256, 256)).to(dev)
        kw = dict(c2ws=c2ws, intrinsics=intr, image_attrs=images, perspective=True, H=256, W=256, H2D=512, W2D=512,
                  filt_gradient_points=True, ray_normal_angle_threhold=115.0, return_layers=True)
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
            res["winner_equal"] = bool(torch.equal(inv.last["winner"], one.last["winner"]))
            res["seen"] = float((one.last["winner"] >= 0).float().mean())
        dist.barrier()
        if rank == 0:
            q.put(res)
    finally:
        dist.destroy_process_group()


def test_view_sharded_perspective_infer_is_bit_identical_to_one_rank():
    """two gloo ranks on one GPU, each back-projecting three perspective views (eyes indexed by absolute view id, as dirs are)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29910 + (os.getpid() % 30)
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res["seen"] > 0.05
    for k, v in res.items():
        if k.endswith("_equal"):
            assert v, "%s differs between world=2 and world=1: %s" % (k, res)
