"""Atlas-space geometry buffers on the GPU: utx_uv_gbuffer / ops.uv_gbuffer / NVDiffRendererInverse.simple_inverse_rendering against the
reference's own buffers (fixture G17), against the existing per-buffer kernels, and at the edges.  Bounds: the docstring of
oracle/gbuffer_ref.py -- bit-exact for mask, alpha and the pure interpolations, 5u for the two normal buffers (the project's bound, G13),
5u * d / 7u / 20u for distance / ray_direction / cos_ray_normal, the matmul-order terms added end to end.  Against the float32 numpy restatement,
which is written in the kernel's operation order with correctly rounded operations, EVERY buffer is bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import gbuffer_ref as GB

pytestmark = pytest.mark.gpu
F32 = np.float32
(H, W), B = GB.ATLAS, GB.VIEWS
ALL = ("mask", "alpha") + GB.WORLD + GB.PER_VIEW


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _against_fixture(name, got, f, tag, own_attrs=False, keys=ALL):
    ref = GB.fixture_buffers(f, tag)
    cov = ref["mask"]
    for k in keys:
        if k == "mask":
            assert np.array_equal(got[k].reshape(cov.shape).astype(bool), cov), name
        elif k == "alpha":
            assert got[k].reshape(ref[k].shape).tobytes() == ref[k].tobytes(), name
        else:
            GB.check("%s %s %s" % (name, k, tag), got[k], ref[k], GB.bounds(k, ref["distance"], own_attrs=(f, tag) if own_attrs else None), cov)


def _against_restatement(name, got, rast, faces, v_pos=None, v_nrm=None, v_pos_cam=None, v_nrm_cam=None):
    want = GB.table(rast, faces, v_pos, v_nrm, v_pos_cam, v_nrm_cam)
    for k, g in got.items():
        w = want[k].astype(np.uint8) if k == "mask" else want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (name, k, g.shape, w.shape)
        assert np.isfinite(g).all(), (name, k)
        assert g.tobytes() == w.tobytes(), "%s %s: max|diff| %.3g" % (name, k, np.abs(g.astype(np.float64) - w).max())


@pytest.mark.parametrize("tag", GB.SETS)
def test_g17_uv_gbuffer_on_fixture_raster_and_arrays(tag):
    """one launch, every buffer, on the reference's raster and the per-vertex arrays it handed to dr.interpolate; the zero-length vertex
    normal (0 / 1e-12 = 0 in camera space) stays finite and equal"""
    from unitex_amd.texturetools import ops
    f = GB.load_g17()
    out = ops.uv_gbuffer(_cu(f["rast"]), _cu(f["faces"], torch.int32), _cu(f["verts"]), _cu(f["v_nrm"]), want=ALL,
                         v_pos_cam=_cu(f["v_pos_cam_" + tag]), v_nrm_cam=_cu(f["v_nrm_cam_" + tag]))
    assert out["mask"].dtype == torch.uint8 and tuple(out["mask"].shape) == GB.ATLAS and tuple(out["alpha"].shape) == (H, W, 1)
    got = _np(out)
    assert all(np.isfinite(v).all() for v in got.values())
    _against_fixture("direct", got, f, tag)
    _against_restatement("direct " + tag, got, f["rast"], f["faces"], f["verts"], f["v_nrm"], f["v_pos_cam_" + tag], f["v_nrm_cam_" + tag])


def _write_obj(path, verts, faces, uvs):
    with open(path, "w") as fh:       # nine significant digits: float32 survives the text
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(v) for v in verts) + "".join("vt %.9g %.9g\n" % tuple(t) for t in uvs))
        fh.write("".join("f %d/%d %d/%d %d/%d\n" % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1) for a, b, c in faces))


@pytest.mark.parametrize("tag", GB.SETS)
def test_g17_simple_inverse_rendering_end_to_end(tag, tmp_path):
    """update_from_file on a temporary .obj, own UV raster (equal to the fixture's in (u, v, id): the precondition of every bound), own w2c,
    utx_transform_points and utx_camera_normals: the reference's keys, shapes and dtypes, the world buffers as in the direct test and the
    camera-dependent ones with the matmul-order terms"""
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    f = GB.load_g17()
    _write_obj(str(tmp_path / "m.obj"), f["verts"], f["faces"], f["uvs"])
    inv = NVDiffRendererInverse(device="cuda:0").update_from_file(str(tmp_path / "m.obj"))
    m = inv.pbr_mesh
    assert np.array_equal(m.vertices.cpu().numpy(), f["verts"]) and np.array_equal(m.faces.cpu().numpy(), f["faces"]) and np.array_equal(m.uvs01, f["uvs"])
    m.set_vertex_normals(f["v_nrm"])
    assert np.array_equal(inv._uv_raster(*GB.ATLAS).cpu().numpy()[..., [0, 1, 3]], f["rast"][..., [0, 1, 3]])
    flags = {"render_" + k: True for k in GB.WORLD + GB.PER_VIEW}
    out = inv.simple_inverse_rendering(torch.from_numpy(f["c2ws_" + tag]), GB.ATLAS, **flags)
    assert sorted(out) == sorted(ALL)
    assert out["mask"].dtype == torch.bool and tuple(out["mask"].shape) == (1, H, W, 1)
    assert out["alpha"].dtype == torch.float32 and tuple(out["alpha"].shape) == (1, H, W, 1)
    for k in GB.WORLD + GB.PER_VIEW:
        assert out[k].dtype == torch.float32 and tuple(out[k].shape) == (B if k in GB.PER_VIEW else 1, H, W, GB.CHANNELS[k]), k
    got = _np(out)
    got["alpha"] = got["alpha"][0]
    _against_fixture("end to end", got, f, tag, own_attrs=True)
    # without cameras: the camera-independent keys only, the same values; enable_antialis changes nothing; compute_uv_mask is mask[0]
    none = inv.simple_inverse_rendering(None, GB.ATLAS, render_world_normal=True, render_world_position=True, enable_antialis=False)
    assert sorted(none) == ["alpha", "mask", "world_normal", "world_position"]
    for k in none:
        assert torch.equal(none[k], out[k]), k
    assert np.array_equal(none["world_position"].cpu().numpy(), f["none_world_position"])
    assert sorted(inv.simple_inverse_rendering(texture_size=GB.ATLAS)) == ["alpha", "mask"]
    cm = inv.compute_uv_mask(GB.ATLAS)
    assert cm.dtype == torch.bool and tuple(cm.shape) == (H, W, 1) and torch.equal(cm, out["mask"][0])
    assert tuple(inv.compute_uv_mask(24).shape) == (24, 24, 1)


def test_fused_kernel_equals_the_existing_per_buffer_kernels():
    """64 x 56 atlas, B = 2: every buffer bit for bit what callers could already compute -- ops.rasterize -> ops.interpolate for the pure
    interpolations, utx_gbuffer_shade's arms (the existing device routines for normalize and the norm) for the rest, and the dot product
    written with torch's float32 elementwise operations (one rounding each, no contraction) in the kernel's order"""
    from unitex_amd.texturetools import camera, ops
    f = GB.load_g17()
    Hh, Ww, n = 64, 56, 2
    faces, vd, nd = _cu(f["faces"], torch.int32), _cu(f["verts"]), _cu(f["v_nrm"])
    uv = _cu(f["uvs"]) * 2.0 - 1.0
    rast = ops.rasterize(torch.cat([uv, torch.zeros_like(uv[:, :1]), torch.ones_like(uv[:, :1])], -1).contiguous(), faces, Hh, Ww)
    cov = rast[..., 3] > 0
    assert cov.any() and not cov.all()
    c2ws = torch.from_numpy(f["c2ws_o"][:n])
    out = ops.uv_gbuffer(rast, faces, vd, nd, c2ws=c2ws, want=ALL)
    pcam = ops.transform_points(vd, camera.c2w_to_w2c(c2ws).cuda().contiguous(), want_ndc=False)[0][..., :3].contiguous()
    ncam = ops.camera_normals(nd, c2ws.cuda().contiguous())
    raw = lambda mode, attr: ops.gbuffer_shade(mode, rast, faces, attr, scale2=None, ndc=False, bg=None, want_rgba=True)[1]
    sel = lambda x, fill: torch.where(cov[..., None], x, torch.full_like(x, fill))
    assert torch.equal(out["mask"], cov.to(torch.uint8)) and torch.equal(out["alpha"], cov.float()[..., None])
    assert torch.equal(out["world_position"][0], sel(ops.interpolate(vd, rast, faces), -1.0))
    assert torch.equal(out["world_normal"][0], raw("world_normal", nd)[..., :3])
    for b in range(n):
        assert torch.equal(out["camera_position"][b], ops.interpolate(pcam[b].contiguous(), rast, faces)), b
        assert torch.equal(out["z_depth"][b], ops.interpolate(pcam[b, :, 2:].contiguous(), rast, faces)), b
        cn, rd = raw("camera_normal", ncam[b])[..., :3], raw("world_normal", pcam[b])[..., :3]      # the normal arm on positions: normalize(interp), -1
        assert torch.equal(out["camera_normal"][b], cn) and torch.equal(out["ray_direction"][b], rd), b
        assert torch.equal(out["distance"][b], raw("distance", pcam[b])[..., :1]), b
        cos = (cn[..., 0:1] * rd[..., 0:1] + cn[..., 1:2] * rd[..., 1:2]) + cn[..., 2:3] * rd[..., 2:3]
        assert torch.equal(out["cos_ray_normal"][b], sel(cos, -1.0)), b


def _abi(ctx, rast, faces, v_pos, v_nrm, v_pos_cam, v_nrm_cam, V, B, Hh, Ww, want, outs):
    from unitex_amd._lib import ptr
    from unitex_amd.texturetools import ops
    ptrs = (C.c_void_p * len(ops.UV_GBUFFERS))()
    for k, t in outs.items():
        ptrs[ops.UV_GBUFFERS[k][0]] = t.data_ptr() if t is not None else None
    bits = sum(1 << ops.UV_GBUFFERS[k][0] for k in want)
    return ctx.lib.utx_uv_gbuffer(ctx.handle, ptr(rast), ptr(faces), ptr(v_pos), ptr(v_nrm), ptr(v_pos_cam), ptr(v_nrm_cam), V, B, Hh, Ww, bits, ptrs,
                                  ctx.stream())


def test_edges():
    from unitex_amd.flux.ops import get_ctx
    from unitex_amd.texturetools import ops
    f = GB.load_g17()
    faces, vd, nd = _cu(f["faces"], torch.int32), _cu(f["verts"]), _cu(f["v_nrm"])
    pc, nc = f["v_pos_cam_p"], f["v_nrm_cam_p"]
    uvclip = lambda uvs: torch.cat([_cu(uvs) * 2.0 - 1.0, torch.zeros(len(uvs), 1, device="cuda"), torch.ones(len(uvs), 1, device="cuda")], -1).contiguous()
    # an atlas whose sides are no multiple of the block (33 x 17 = 561 texels: two full blocks and a ragged third), B = 1
    rast = ops.rasterize(uvclip(f["uvs"]), faces, 33, 17)
    got = _np(ops.uv_gbuffer(rast, faces, vd, nd, want=ALL, v_pos_cam=_cu(pc[:1]), v_nrm_cam=_cu(nc[:1])))
    assert got["camera_normal"].shape == (1, 33, 17, 3) and got["mask"].any() and not got["mask"].all()
    _against_restatement("33 x 17, B = 1", got, rast.cpu().numpy(), f["faces"], f["verts"], f["v_nrm"], pc[:1], nc[:1])
    # B = 0: camera-independent buffers only; a camera-dependent one comes back empty, nothing is launched for it
    out = ops.uv_gbuffer(rast, faces, vd, nd, c2ws=torch.zeros(0, 4, 4), want=("mask", "world_normal", "world_position", "distance"))
    assert tuple(out["distance"].shape) == (0, 33, 17, 1)
    _against_restatement("B = 0", _np({k: out[k] for k in ("mask", "world_normal", "world_position")}), rast.cpu().numpy(), f["faces"], f["verts"], f["v_nrm"])
    # no covered texel: every background, no NaN
    empty = torch.zeros(H, W, 4, device="cuda")
    got = _np(ops.uv_gbuffer(empty, faces, vd, nd, want=ALL, v_pos_cam=_cu(pc), v_nrm_cam=_cu(nc)))
    for k in ALL:
        fill = 0.0 if k in ("mask", "alpha") else GB.FILL[k]
        assert np.isfinite(got[k]).all() and (got[k] == fill).all(), k
    # a UV triangle without area (its three uvs on one line) next to the charts: it covers nothing it should not, and everything stays finite
    uvs2 = np.concatenate([f["uvs"], np.array([[0.5, 0.2], [0.5, 0.5], [0.5, 0.8]], F32)])
    verts2 = np.concatenate([f["verts"], np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0]], F32)])
    nrm2 = np.concatenate([f["v_nrm"], np.zeros((3, 3), F32)])
    V = len(f["verts"])
    faces2 = np.concatenate([f["faces"], np.array([[V, V + 1, V + 2]], np.int32)])
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], 3, 3), F32)], 1)
    rast2 = ops.rasterize(uvclip(uvs2), _cu(faces2, torch.int32), H, W)
    assert np.array_equal(rast2.cpu().numpy()[..., [0, 1, 3]], f["rast"][..., [0, 1, 3]])
    got = _np(ops.uv_gbuffer(rast2, _cu(faces2, torch.int32), _cu(verts2), _cu(nrm2), want=ALL, v_pos_cam=_cu(pad(pc)), v_nrm_cam=_cu(pad(nc))))
    _against_fixture("degenerate UV triangle", got, f, "p")
    # a single requested buffer: the words around it, and the buffers of every other bit (valid pointers, not requested), keep their sentinel
    ctx = get_ctx(0)
    npix, SENT = H * W, -77.0
    rastd = _cu(f["rast"])
    guard = torch.full((3 * B * npix + 512,), SENT, device="cuda")
    others = {k: torch.full((B * npix * 3,), SENT, device="cuda") for k in ALL if k not in ("mask", "ray_direction")}
    others["mask"] = torch.full((npix,), 77, dtype=torch.uint8, device="cuda")
    outs = dict(others, ray_direction=guard[256:256 + 3 * B * npix])
    assert _abi(ctx, rastd, faces, None, None, _cu(pc), None, V, B, H, W, ("ray_direction",), outs) == 0
    torch.cuda.synchronize()
    assert (guard[:256] == SENT).all() and (guard[256 + 3 * B * npix:] == SENT).all()
    assert np.array_equal(guard[256:256 + 3 * B * npix].view(B, H, W, 3).cpu().numpy(),
                          GB.table(f["rast"], f["faces"], v_pos_cam=pc)["ray_direction"])
    for k, t in others.items():
        assert (t == (77 if k == "mask" else SENT)).all(), k


def test_export_uv_maps(tmp_path):
    from PIL import Image
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    f = GB.load_g17()
    inv = NVDiffRendererInverse(device="cuda:0").update_from_arrays(f["verts"], f["faces"], f["uvs"])
    inv.pbr_mesh.set_vertex_normals(f["v_nrm"])
    paths = inv.export_uv_maps(str(tmp_path / "maps"), texture_size=GB.ATLAS)
    assert [os.path.basename(p) for p in paths] == ["uv_mask.png", "uv_position.png", "uv_normal.png"]
    mask, pos, nrm = [Image.open(p) for p in paths]
    assert mask.mode == "L" and pos.mode == "RGB" and nrm.mode == "RGB" and mask.size == pos.size == nrm.size == (W, H)
    cov = f["mask"][..., 0] > 0
    mask, pos, nrm = np.asarray(mask), np.asarray(pos), np.asarray(nrm)
    assert np.array_equal(mask, np.where(cov[::-1], 255, 0))                        # row 0 of the image is v = 1: the raster's last row
    assert not np.array_equal(cov[::-1], cov)
    assert (pos[~cov[::-1]] == 0).all() and (nrm[~cov[::-1]] == 0).all()            # -1 * 0.5 + 0.5
    to_u8 = lambda x: (np.clip(x * F32(0.5) + F32(0.5), F32(0), F32(1)) * F32(255.0)).astype(np.uint8)
    assert np.array_equal(pos, to_u8(f["world_position"][0])[::-1])                  # bit-exact buffer -> equal bytes
    assert np.abs(nrm.astype(np.int32) - to_u8(f["world_normal"][0])[::-1]).max() <= 1


def test_error_codes_through_the_c_abi():
    """argument checks in front of the launch: a negative code and a message in utx_last_error, nothing reaches the device"""
    from unitex_amd.flux.ops import get_ctx
    f = GB.load_g17()
    ctx = get_ctx(0)
    V, npix = len(f["verts"]), H * W
    rast, faces, vd, nd = _cu(f["rast"]), _cu(f["faces"], torch.int32), _cu(f["verts"]), _cu(f["v_nrm"])
    pc, nc = _cu(f["v_pos_cam_p"]), _cu(f["v_nrm_cam_p"])
    bufs = {"world_position": torch.empty(npix * 3, device="cuda"), "z_depth": torch.empty(B * npix, device="cuda"),
            "camera_normal": torch.empty(B * npix * 3, device="cuda")}
    call = lambda **kw: _abi(ctx, **dict(dict(rast=rast, faces=faces, v_pos=vd, v_nrm=nd, v_pos_cam=pc, v_nrm_cam=nc, V=V, B=B, Hh=H, Ww=W,
                                              want=("world_position", "z_depth", "camera_normal"), outs=bufs), **kw))
    assert call() == 0
    bad = [dict(outs=dict(bufs, z_depth=None)),                 # a requested buffer without a pointer
           dict(v_pos_cam=None), dict(v_nrm_cam=None),          # a camera-dependent request without its per-view array
           dict(v_pos=None), dict(rast=None), dict(faces=None), dict(Hh=0), dict(Ww=-1), dict(B=-1), dict(V=0), dict(want=())]
    for kw in bad:
        assert call(**kw) == -2, kw
        assert b"utx_uv_gbuffer" in ctx.lib.utx_last_error(ctx.handle), kw
    assert call(rast=rast.view(-1)[1:]) == -2                   # read as float4: off a 16-byte boundary
    assert ctx.lib.utx_uv_gbuffer(ctx.handle, C.c_void_p(rast.data_ptr()), C.c_void_p(faces.data_ptr()), None, None, None, None, V, 0, H, W, 1 << 10,
                                  (C.c_void_p * 10)(), ctx.stream()) == -2      # an unknown bit
    assert call(v_pos_cam=None, v_nrm_cam=None, B=0, want=("world_position",)) == 0      # B = 0 needs no per-view array
    torch.cuda.synchronize()
