"""The atlas kernel (utx_uv_gbuffer) and the screen kernel (utx_screen_gbuffer) compute the same per-pixel geometry: on the same raster, repeated
once per view, with the same per-view vertex arrays, every buffer they share is equal bit for bit.  z_depth is the one buffer that differs by
design -- camera z on the atlas, the interpolated clip w on the screen -- and each is checked against its own definition.  Uncovered texels hold
the background of the table in csrc/gbuffer.hip in both.

The mesh is small enough to reason about: a UV-mapped quad of two triangles (their common edge crosses the raster diagonally) and one detached
triangle that reaches past the right border, on a 17 x 19 atlas = 323 texels, two blocks of 256 with the second one ragged.  The per-view vertex
arrays are handed in, so no camera code runs."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 17, 19
SHARED = ("mask", "alpha", "world_normal", "world_position", "camera_normal", "camera_position", "distance", "ray_direction", "cos_ray_normal")
ALL = SHARED + ("z_depth",)
CHANNELS = dict(mask=1, alpha=1, world_normal=3, world_position=3, camera_normal=3, camera_position=3, distance=1, ray_direction=3, cos_ray_normal=1,
                z_depth=1)
FILL = dict(mask=0, alpha=0.0, world_normal=-1.0, world_position=-1.0, camera_normal=-1.0, camera_position=0.0, distance=0.0, ray_direction=-1.0,
            cos_ray_normal=-1.0, z_depth=0.0)      # the background column of the table in csrc/gbuffer.hip
GUARD, SENT = 64, -77.0


def _scene(B):
    from unitex_amd.texturetools import ops
    rng = np.random.RandomState(7)
    uvs = np.array([[0.06, 0.10], [0.58, 0.14], [0.55, 0.90], [0.08, 0.84], [0.70, 0.20], [1.20, 0.45], [0.74, 0.80]], np.float32)
    cu = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()
    s = dict(faces=cu(np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]]), torch.int32), v_pos=cu(rng.uniform(-1, 1, (7, 3))), v_nrm=cu(rng.normal(size=(7, 3))),
             v_pos_cam=cu(rng.uniform(-2, 2, (B, 7, 3))), v_nrm_cam=cu(rng.normal(size=(B, 7, 3))))
    uv = cu(uvs) * 2.0 - 1.0
    s["rast2d"] = ops.rasterize(torch.cat([uv, torch.zeros_like(uv[:, :1]), torch.ones_like(uv[:, :1])], -1).contiguous(), s["faces"], H, W)
    s["rast"] = s["rast2d"][None].expand(B, H, W, 4).contiguous()
    s["clip_w"] = s["v_pos_cam"][..., 2].contiguous()
    ids = s["rast2d"][..., 3]
    assert sorted(ids.unique().tolist()) == [0.0, 1.0, 2.0, 3.0] and bool((ids[:, W - 1] == 3).any())      # uncovered texels, every triangle, the border
    return s


def _guarded(n, dtype):
    """n elements between GUARD sentinel elements on either side: (the whole allocation, the payload)"""
    t = torch.full((n + 2 * GUARD,), 77 if dtype == torch.uint8 else SENT, dtype=dtype, device="cuda")
    return t, t[GUARD:GUARD + n]


def _raw(entry, table, s, B, want):
    """the raw entry point into guarded buffers: {name: flat payload}, after checking that every guard element kept its sentinel"""
    from unitex_amd._lib import ptr
    from unitex_amd.flux.ops import get_ctx
    ctx = get_ctx(0)
    layers = lambda k: 1 if entry == "uv" and k in ("mask", "alpha", "world_normal", "world_position") else B
    bufs = {k: _guarded(layers(k) * H * W * CHANNELS[k], torch.uint8 if k == "mask" else torch.float32) for k in want}
    ptrs = (C.c_void_p * len(table))()
    for k, (_, payload) in bufs.items():
        ptrs[table[k][0]] = payload.data_ptr()
    bits = sum(1 << table[k][0] for k in want)
    a = [ptr(s["rast2d"] if entry == "uv" else s["rast"]), ptr(s["faces"]), ptr(s["v_pos"]), ptr(s["v_nrm"])]
    if entry == "uv":
        rc = ctx.lib.utx_uv_gbuffer(ctx.handle, *a, ptr(s["v_pos_cam"]), ptr(s["v_nrm_cam"]), 7, B, H, W, bits, ptrs, ctx.stream())
    else:
        rc = ctx.lib.utx_screen_gbuffer(ctx.handle, *a, None, None, 0, ptr(s["clip_w"]), ptr(s["v_pos_cam"]), ptr(s["v_nrm_cam"]), 7, B, H, W, 0, None,
                                        (C.c_int * 1)(), 0, 0, 0.0, None, None, bits, ptrs, ctx.stream())
    assert rc == 0, ctx.lib.utx_last_error(ctx.handle)
    torch.cuda.synchronize()
    for k, (whole, payload) in bufs.items():
        fill = 77 if k == "mask" else SENT
        assert bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + payload.numel():] == fill).all()), (entry, k)
    return {k: payload for k, (_, payload) in bufs.items()}


@pytest.mark.parametrize("B,want", [(3, ALL), (1, ALL), (3, ("cos_ray_normal",))], ids=["B3-all", "B1-all", "B3-cos_ray_normal-only"])
def test_atlas_and_screen_kernels_compute_the_same_buffers(B, want):
    from unitex_amd.texturetools import ops
    s = _scene(B)
    atlas = ops.uv_gbuffer(s["rast2d"], s["faces"], s["v_pos"], s["v_nrm"], want=want, v_pos_cam=s["v_pos_cam"], v_nrm_cam=s["v_nrm_cam"])
    screen = ops.screen_gbuffer(s["rast"], s["faces"], s["v_pos"], v_nrm=s["v_nrm"], want=want, clip_w=s["clip_w"], v_pos_cam=s["v_pos_cam"],
                                v_nrm_cam=s["v_nrm_cam"])
    assert sorted(atlas) == sorted(screen) == sorted(want)
    cov = s["rast2d"][..., 3] > 0
    for k in want:
        assert bool(torch.isfinite(atlas[k].float()).all()), k
        assert bool((screen[k][:, ~cov] == FILL[k]).all()) and bool((atlas[k].reshape(-1, H, W, CHANNELS[k])[:, ~cov] == FILL[k]).all()), k
        if k == "z_depth":
            continue
        a = atlas[k]
        if k == "mask":                       # uint8 [H,W] on the atlas, uint8 [B,H,W] on the screen
            assert a.dtype == screen[k].dtype == torch.uint8
            a = a[None].expand(B, H, W)
        elif k == "alpha":                    # [H,W,1] against [B,H,W,1]
            a = a[None].expand(B, H, W, 1)
        elif k.startswith("world_"):          # [1,H,W,3] against [B,H,W,3]
            a = a.expand(B, H, W, 3)
        assert tuple(screen[k].shape) == tuple(a.shape) and torch.equal(screen[k], a), k
    if "cos_ray_normal" in want:              # not the background everywhere: the covered texels carry a dot product of two unit vectors
        c = atlas["cos_ray_normal"][:, cov]
        assert bool((c != -1.0).any()) and bool((c.abs() <= 1.0 + 1e-6).all())
    if "z_depth" in want:
        assert torch.equal(atlas["z_depth"], atlas["camera_position"][..., 2:])
        for b in range(B):
            w = ops.interpolate(s["clip_w"][b][:, None].contiguous(), s["rast2d"], s["faces"])
            assert torch.equal(screen["z_depth"][b], torch.where(cov[..., None], w, torch.zeros_like(w))), b
    # the same launches through the raw entry points, every output between sentinels: nothing written outside, the same bits inside
    for entry, table, got in (("uv", ops.UV_GBUFFERS, atlas), ("screen", ops.SCREEN_GBUFFERS, screen)):
        raw = _raw(entry, table, s, B, want)
        for k in want:
            assert torch.equal(raw[k], got[k].reshape(-1)), (entry, k)
