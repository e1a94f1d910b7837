"""Geometry-buffer video types of VideoExporter.export_orbit_video on the GPU: utx_gbuffer_shade / utx_gbuffer_range / utx_camera_normals
against the reference's own frames (fixture G13) and, at production size, against the numpy restatement of oracle/video_types_ref.py
(which that module proves against the same fixture).  Bounds: see that module's docstring -- bit-exact for the position and depth arms,
derived ulp bounds where torch's own norm / matmul order enters; against the restatement, which is written in the kernels' operation order
with correctly rounded numpy operations, EVERY arm is bit-exact."""
import os

import numpy as np
import pytest
import torch

from oracle import video_types_ref as VC

pytestmark = pytest.mark.gpu
F32 = np.float32
GEOM_TYPES, NORMALIZE, SETS = VC.GEOM_TYPES, VC.NORMALIZE, VC.SETS


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _mesh(f):
    return (f["verts"], f["faces"], f["uvs"], f["tex"], f["v_nrm"])


@pytest.mark.parametrize("video_type", GEOM_TYPES)
def test_g13_gbuffer_shade_on_fixture_rast(video_type):
    """ops.gbuffer_shade / gbuffer_range on the reference's rast and per-vertex attributes: float RGBA and uint8 frames of every type, both
    camera models; (lo, hi) of z_depth bit for bit (distance: two norms, 5u, as in the CPU module)"""
    from unitex_amd.texturetools import ops
    f = VC.load()
    faces = _cu(f["faces"], torch.int32)
    for tag, (persp, n, size) in SETS.items():
        ref, alpha = VC.fixture_frames(f, video_type, tag), f["alpha_" + tag]
        scale = None
        if video_type in NORMALIZE:
            want = f["scale_%s_%s" % (video_type, tag)]
            s3 = ops.gbuffer_range(video_type, _cu(f["rast_" + tag][0]), faces, _cu(VC.fixture_attr(f, video_type, tag, 0)))
            got, empty = s3[:2].cpu().numpy(), int(s3.cpu().view(torch.int32)[2])
            print("%s %s (lo, hi): %r, reference %r, empty %d" % (video_type, tag, tuple(got), tuple(want), empty))
            assert empty == 0
            if video_type == "z_depth":
                assert got.tobytes() == want.tobytes()
            else:
                assert np.all(np.abs(got.astype(np.float64) - want) <= 5 * VC.U * want[1])
                assert got.tobytes() == np.asarray(VC.value_range(video_type, f["rast_" + tag][0], f["faces"], VC.fixture_attr(f, video_type, tag, 0)), F32).tobytes()
            scale = _cu(want)        # the reference's pair, so that the frames are compared on identical inputs
        for i in range(n):
            u8, rgba = ops.gbuffer_shade(video_type, _cu(f["rast_" + tag][i]), faces, _cu(VC.fixture_attr(f, video_type, tag, i)), scale2=scale,
                                         ndc=video_type not in NORMALIZE, bg=(1.0, 1.0, 1.0), want_rgba=True)
            VC.check_frame("%s %s[%d]" % (video_type, tag, i), rgba.cpu().numpy(), u8.cpu().numpy(), ref[i], alpha[i], VC.float_bound(f, video_type, tag))
            assert np.array_equal(ops.gbuffer_shade(video_type, _cu(f["rast_" + tag][i]), faces, _cu(VC.fixture_attr(f, video_type, tag, i)), scale2=scale,
                                                    ndc=video_type not in NORMALIZE).cpu().numpy(), u8.cpu().numpy())      # without the float frame


def test_g13_frame_outside_first_frame_range_is_reproduced():
    """frame 1 of the perspective set reaches depths on both sides of frame 0's (lo, hi): the float frame leaves [0, 1] exactly as the
    reference's does and the uint8 one is clamped"""
    from unitex_amd.texturetools import ops
    f = VC.load()
    faces = _cu(f["faces"], torch.int32)
    attr = _cu(VC.fixture_attr(f, "z_depth", "p", 1))
    u8, rgba = ops.gbuffer_shade("z_depth", _cu(f["rast_p"][1]), faces, attr, scale2=_cu(f["scale_z_depth_p"]), bg=(1.0, 1.0, 1.0), want_rgba=True)
    rgba, u8, cov = rgba.cpu().numpy(), u8.cpu().numpy(), f["alpha_p"][1] > 0
    assert rgba[..., 0][cov].min() < 0.0 and rgba[..., 0][cov].max() > 1.0
    assert np.array_equal(rgba[..., 0], f["z_depth_p"][1])
    assert (u8[..., 0][cov & (rgba[..., 0] < 0)] == 0).all() and (u8[..., 0][cov & (rgba[..., 0] > 1)] == 255).all()


@pytest.mark.parametrize("perspective", [True, False])
@pytest.mark.parametrize("video_type", GEOM_TYPES)
def test_g13_export_orbit_video_end_to_end(video_type, perspective, tmp_path):
    """export_orbit_video with its own cameras, transform, rasteriser and per-vertex kernels.  Its rast equals the fixture's in (u, v, id)
    (asserted: the precondition of every bound), so world_position and z_depth stay bit-exact and the others carry the bounds derived for
    per-vertex attributes recomputed in the build's order (CPU module docstring)."""
    from unitex_amd.texturetools import camera, ops
    from unitex_amd.texturetools.video import VideoExporter
    f = VC.load()
    tag = "p" if perspective else "o"
    _, n, size = SETS[tag]
    mvp = torch.matmul(camera.intr_to_proj(torch.from_numpy(f["intr_" + tag]), perspective=perspective), camera.c2w_to_w2c(torch.from_numpy(f["c2ws_" + tag]))).cuda().contiguous()
    clip, _ = ops.transform_points(_cu(f["verts"]), mvp, want_ndc=False)
    for i in range(n):
        r = ops.rasterize(clip[i].contiguous(), _cu(f["faces"], torch.int32), size, size).cpu().numpy()
        assert np.array_equal(r[..., [0, 1, 3]], f["rast_" + tag][i][..., [0, 1, 3]])
    ex = VideoExporter(device="cuda:0")
    kw = dict(n_frames=n, perspective=perspective, video_type=video_type, render_size=size, save_camera=True)
    rgba = ex.export_orbit_video(_mesh(f), str(tmp_path / "a.mp4"), return_frames="rgba", **kw)
    u8 = ex.export_orbit_video(_mesh(f), str(tmp_path / "a.mp4"), return_frames=True, **kw)
    cam = torch.load(str(tmp_path / "a_camera.pth"))
    assert np.array_equal(cam["c2ws"].numpy(), f["c2ws_" + tag]) and np.array_equal(cam["intrinsics"].numpy(), f["intr_" + tag])
    assert len(rgba) == n and len(u8) == n and u8[0].dtype == np.uint8 and u8[0].shape == (size, size, 3)
    ref, alpha = VC.fixture_frames(f, video_type, tag), f["alpha_" + tag]
    for i in range(n):
        VC.check_frame("%s %s[%d] end to end" % (video_type, tag, i), rgba[i], u8[i], ref[i], alpha[i], VC.float_bound(f, video_type, tag, own_attrs=True))


@pytest.mark.parametrize("perspective", [True, False])
def test_g13_rgb_turntable_end_to_end(perspective, tmp_path):
    """the seventh type: export_orbit_video(video_type='rgb') against the reference's own export_video frames, both camera models; uint8
    against trunc(clamp(x) * 255) of the reference's float frame with the near-integer rule at RGB_ULPS (derived in the CPU module)"""
    from unitex_amd.texturetools.video import VideoExporter
    f = VC.load()
    tag = "p" if perspective else "o"
    _, n, size = SETS[tag]
    mesh = (f["verts"], f["faces"], f["uvs"], np.ascontiguousarray(f["tex"][::-1]), f["v_nrm"])     # the tuple's image is top-down: row 0 = v = 1
    frames = VideoExporter(device="cuda:0").export_orbit_video(mesh, str(tmp_path / "rgb.mp4"), n_frames=n, perspective=perspective, video_type="rgb",
                                                               render_size=size, return_frames=True)
    assert len(frames) == n
    for i in range(n):
        VC.check_u8("rgb %s[%d] end to end" % (tag, i), frames[i], f["rgb_" + tag][i], VC.RGB_ULPS * VC.U)


def test_fused_interpolation_equals_ops_interpolate():
    """world_position / camera_position / z_depth with normalisation, ndc and composite switched off are the interpolated value itself:
    bit-identical to utx_interpolate (background fill where empty), also through a strided attribute view"""
    from unitex_amd.texturetools import ops
    f = VC.load()
    faces, rast = _cu(f["faces"], torch.int32), _cu(f["rast_p"][1])
    cov = (rast[..., 3] > 0).cpu().numpy()
    wide = torch.zeros(f["verts"].shape[0], 4, device="cuda")
    wide[:, :3], wide[:, 3] = _cu(f["verts"]), _cu(f["v_clip_w_p"][1])
    for mode, attr, fill in (("world_position", _cu(f["verts"]), -1.0), ("camera_position", wide[:, :3], 0.0), ("z_depth", wide[:, 3:], 0.0)):
        want = ops.interpolate(attr.contiguous(), rast, faces).cpu().numpy()
        _, rgba = ops.gbuffer_shade(mode, rast, faces, attr, scale2=None, ndc=False, bg=None, want_rgba=True)
        got = rgba.cpu().numpy()
        assert np.array_equal(got[..., :3][cov], np.broadcast_to(want, got[..., :3].shape)[cov]), mode
        assert (got[..., :3][~cov] == fill).all() and np.array_equal(got[..., 3], cov.astype(F32))


def test_production_size_against_restatement():
    """1024^2, 20 k faces, 3 perspective frames per type: per-vertex kernels, (lo, hi) and every frame bit-exact against the numpy restatement"""
    from unitex_amd.texturetools import camera, meshes, ops
    verts, faces, _ = meshes.sphere_with_faces(20000)
    verts = (verts * np.array([0.9, 0.6, 0.75], F32) + np.array([0.05, -0.1, 0.2], F32)).astype(F32)
    assert faces.shape[0] >= 20000
    nrm = (verts / np.linalg.norm(verts, axis=-1, keepdims=True)).astype(F32)
    S, n = 1024, 3
    c2ws = camera.generate_orbit_views_c2ws(7, radius=2.8, height=0.7, theta_0=0.0, degree=True)[[0, 2, 5]].float().contiguous()
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    vd, fd, nd = _cu(verts), _cu(faces, torch.int32), _cu(nrm)
    w2c_h = camera.c2w_to_w2c(c2ws).float().contiguous()
    mvp_h = torch.matmul(camera.intr_to_proj(intr, perspective=True), w2c_h).contiguous()
    clip, _ = ops.transform_points(vd, mvp_h.cuda(), want_ndc=False)
    cam, _ = ops.transform_points(vd, w2c_h.cuda(), want_ndc=False)
    ncam = ops.camera_normals(nd, c2ws.cuda())
    rasts = [ops.rasterize(clip[i].contiguous(), fd, S, S) for i in range(n)]
    rasts_h = [r.cpu().numpy() for r in rasts]
    gpu_attr = {"world_normal": lambda i: nd, "camera_normal": lambda i: ncam[i], "world_position": lambda i: vd,
                "camera_position": lambda i: cam[i, :, :3], "z_depth": lambda i: clip[i, :, 3:], "distance": lambda i: cam[i, :, :3]}
    for t in GEOM_TYPES:
        attrs = [VC.vertex_attr(t, verts, nrm, c2ws[i].numpy(), intr.numpy(), True, w2c=w2c_h[i].numpy(), mvp=mvp_h[i].numpy()) for i in range(n)]
        scale_h = scale_d = None
        for i in range(n):
            assert np.array_equal(gpu_attr[t](i).cpu().numpy(), attrs[i]), "%s: per-vertex attribute of frame %d" % (t, i)
        if t in NORMALIZE:
            scale_h = np.asarray(VC.value_range(t, rasts_h[0], faces, attrs[0]), F32)
            s3 = ops.gbuffer_range(t, rasts[0], fd, gpu_attr[t](0))
            assert s3[:2].cpu().numpy().tobytes() == scale_h.tobytes() and int(s3.cpu().view(torch.int32)[2]) == 0
            scale_d = s3[:2]
        for i in range(n):
            want_rgba, want_u8 = VC.shade(t, rasts_h[i], faces, attrs[i], scale2=scale_h, ndc=t not in NORMALIZE)
            u8, rgba = ops.gbuffer_shade(t, rasts[i], fd, gpu_attr[t](i), scale2=scale_d, ndc=t not in NORMALIZE, bg=(1.0, 1.0, 1.0), want_rgba=True)
            VC.check_frame("%s 1024^2 [%d]" % (t, i), rgba.cpu().numpy(), u8.cpu().numpy(), want_rgba[..., :3], want_rgba[..., 3], 0.0)
            assert np.array_equal(u8.cpu().numpy(), want_u8)


def test_rgb_turntable_is_untouched(tmp_path):
    """the new dispatch did not move the rgb path: frames byte-identical to ops.texture_shade on the same rasters"""
    from unitex_amd.texturetools import camera, ops
    from unitex_amd.texturetools.video import VideoExporter
    f = VC.load()
    n, size = 4, 96
    frames = VideoExporter(device="cuda:0").export_orbit_video(_mesh(f)[:4], str(tmp_path / "rgb.mp4"), n_frames=n, render_size=size, return_frames=True)
    c2ws = camera.generate_orbit_views_c2ws(n + 1, radius=2.8, height=0.0, theta_0=0.0, degree=True)[:n]
    intr = camera.generate_intrinsics(49.1, 49.1, fov=True, degree=True)
    mvp = torch.matmul(camera.intr_to_proj(intr, perspective=True), camera.c2w_to_w2c(c2ws)).cuda().contiguous()
    clip, _ = ops.transform_points(_cu(f["verts"]), mvp, want_ndc=False)
    texd = _cu(np.ascontiguousarray(f["tex"][::-1, :, :3]).astype(F32) / F32(255.0))
    for i in range(n):
        rast = ops.rasterize(clip[i].contiguous(), _cu(f["faces"], torch.int32), size, size)
        assert np.array_equal(frames[i], ops.texture_shade(rast, _cu(f["uvs"]), _cu(f["faces"], torch.int32), texd, bg=(1.0, 1.0, 1.0)).cpu().numpy())
    with pytest.raises(AssertionError):
        VideoExporter(device="cuda:0").export_orbit_video(_mesh(f), str(tmp_path / "rgb.mp4"), n_frames=2, render_size=32, return_frames="rgba")


def test_containers_grid_cover_frames_and_enhance_modes(tmp_path):
    from PIL import Image
    from unitex_amd.texturetools.video import VideoExporter, read_mjpeg_mp4
    f = VC.load()
    ex = VideoExporter(device="cuda:0", normal_weighting="area")
    p = str(tmp_path / "n.mp4")
    frames = ex.export_orbit_video(_mesh(f)[:4], p, n_frames=5, video_type="world_normal", render_size=64, fps=12, save_grid=True, save_cover=True,
                                   save_frames=True, return_frames=True)     # no fifth element: _vertex_normals('area')
    fps, jpgs = read_mjpeg_mp4(p)
    assert fps == 12 and len(jpgs) == 5 and len(frames) == 5
    assert np.asarray(Image.open(str(tmp_path / "n_grid.png"))).shape == (3 * 64, 2 * 64, 3)
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "n_cover.png"))), frames[0])
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "n_frames" / "0004.png"))), frames[4])
    assert ex.export_orbit_video(_mesh(f), str(tmp_path / "d.gif"), n_frames=3, video_type="distance", render_size=48, perspective=False) == str(tmp_path / "d.gif")
    g = Image.open(str(tmp_path / "d.gif"))
    assert g.n_frames == 3 and g.size == (48, 48)
    for mode, count in (("pitch", 10), ("box", 6)):
        fr = ex.export_orbit_video(_mesh(f), str(tmp_path / "e.mp4"), n_frames=2, enhance_mode=mode, video_type="z_depth", render_size=32, return_frames=True)
        assert len(fr) == count
    fr = ex.export_orbit_video(_mesh(f), str(tmp_path / "c.mp4"), enhance_mode="canonical", video_type="camera_position", render_size=16, return_frames=True)
    assert len(fr) == 512


def test_empty_first_frame_and_argument_errors(tmp_path):
    from unitex_amd.texturetools import ops
    from unitex_amd.flux.ops import get_ctx
    from unitex_amd.texturetools.video import VideoExporter
    f = VC.load()
    far = (f["verts"] + np.array([0.0, 50.0, 0.0], F32)).astype(F32)        # out of every orbit camera's view
    ex = VideoExporter(device="cuda:0")
    for t in NORMALIZE:
        with pytest.raises(RuntimeError):
            ex.export_orbit_video((far,) + _mesh(f)[1:], str(tmp_path / "e.mp4"), n_frames=2, video_type=t, render_size=32)
    assert len(ex.export_orbit_video((far,) + _mesh(f)[1:], str(tmp_path / "e.mp4"), n_frames=2, video_type="world_normal", render_size=32, return_frames=True)) == 2
    s3 = ops.gbuffer_range("z_depth", torch.zeros(8, 8, 4, device="cuda"), _cu(f["faces"], torch.int32), _cu(f["v_clip_w_p"][0][:, None]))
    assert int(s3.cpu().view(torch.int32)[2]) == 1 and np.isinf(s3[:2].cpu().numpy()).all()
    with pytest.raises(KeyError):
        ex.export_orbit_video(_mesh(f), str(tmp_path / "a.mp4"), video_type="albedo")
    with pytest.raises(AssertionError):
        ex.export_orbit_video(_mesh(f), str(tmp_path / "a.mp4"), video_type="uv")
    # the C ABI refuses a bad mode, null pointers and npix <= 0 with a negative code and a message
    import ctypes as C
    from unitex_amd._lib import ptr
    ctx = get_ctx(0)
    rast, tri, attr = torch.zeros(4, 4, 4, device="cuda"), _cu(f["faces"], torch.int32), _cu(f["verts"])
    out, bg = torch.empty(4, 4, 3, dtype=torch.uint8, device="cuda"), (C.c_float * 3)(1.0, 1.0, 1.0)
    good = lambda: [ctx.handle, 2, ptr(rast), ptr(tri), ptr(attr), 3, ptr(None), 0, bg, 16, ptr(out), ptr(None), ctx.stream()]
    assert ctx.lib.utx_gbuffer_shade(*good()) == 0
    for pos, bad in ((1, 6), (1, -1), (2, ptr(None)), (3, ptr(None)), (4, ptr(None)), (5, 2), (7, 4), (8, None), (9, 0), (10, ptr(None))):
        a = good()
        a[pos] = bad
        assert ctx.lib.utx_gbuffer_shade(*a) < 0, pos
        assert b"utx_gbuffer_shade" in ctx.lib.utx_last_error(ctx.handle)
    # the float4 accesses: a rast or RGBA pointer off a 16-byte boundary is refused, not launched
    rgba = torch.empty(4 * 4 * 4 + 4, device="cuda")
    for pos, bad in ((2, C.c_void_p(rast.data_ptr() + 4)), (11, C.c_void_p(rgba.data_ptr() + 4))):
        a = good()
        a[pos] = bad
        assert ctx.lib.utx_gbuffer_shade(*a) == -2, pos
    a = good()
    a[11] = ptr(rgba)
    assert ctx.lib.utx_gbuffer_shade(*a) == 0
    s3 = torch.empty(3, device="cuda")
    goodr = lambda: [ctx.handle, 4, ptr(rast), ptr(tri), ptr(attr), 3, 16, ptr(s3), C.c_void_p(s3.data_ptr() + 8), ctx.stream()]
    assert ctx.lib.utx_gbuffer_range(*goodr()) == 0
    for pos, bad in ((1, 9), (2, ptr(None)), (2, C.c_void_p(rast.data_ptr() + 4)), (5, 0), (6, 0), (7, ptr(None)), (8, ptr(None))):
        a = goodr()
        a[pos] = bad
        assert ctx.lib.utx_gbuffer_range(*a) < 0, pos
    torch.cuda.synchronize()
