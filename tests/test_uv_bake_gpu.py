"""Blended UV texture bake on the GPU: utx_uv_bake and utx_uv_dilation_step through the C ABI and the wrappers of ops (uv_bake, uv_dilation), and
remapping_uv.project_uv_texture / remapping_uv_texture / uv_dilation against the reference's own arrays (fixture G21) within the counted bounds of
oracle/uv_bake_ref.py.  The kernels are held to the float32 restatement, and utx_uv_bake to the composition of the existing ops, BIT FOR BIT."""
import numpy as np
import pytest
import torch

from oracle import uv_bake_ref as R

pytestmark = pytest.mark.gpu
U = R.U
SENT = 12345.0


def _dev(s):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in s.items()}


def _bake(t, use_alpha=True, epilogue=None):
    from unitex_amd.texturetools import ops
    return ops.uv_bake(t["rast2d"], t["faces"], t["face_mask"], t["v_ndc"], t["images"], t["wmap"], t["rast_view"], t["map_Kd"], t["weights"],
                       use_alpha=use_alpha, epilogue=epilogue)


def _composition(t, use_alpha):
    """project_uv_texture as the existing ops compose it: uv_project with the 6-channel map, then the fp32 elementwise steps in the written order, the views
    added in index order"""
    from unitex_amd.texturetools import ops
    m6 = torch.cat([t["images"].permute(0, 2, 3, 1), t["wmap"]], dim=-1).contiguous()
    p = ops.uv_project(t["rast2d"], t["faces"], t["face_mask"], t["v_ndc"], m6, t["rast_view"], filter="bilinear", background=None)
    rgb, c, e = torch.split(p["map_attr"], [4, 1, 1], dim=-1)
    a = p["uv_alpha"] if use_alpha else torch.ones_like(p["uv_alpha"])
    w = t["weights"][:, None, None, None] * c.square().square() * a * (1 - e)
    col = (a * rgb + (1 - a) * t["map_Kd"]) * w
    acc, wacc = torch.zeros_like(col[0]), torch.zeros_like(w[0])
    for b in range(col.shape[0]):
        acc, wacc = acc + col[b], wacc + w[b]
    return acc, wacc, p


@pytest.mark.parametrize("use_alpha", [True, False])
@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (5, 7, 3, 7), (1, 255, 8, 2), (1, 256, 3, 7), (1, 257, 1, 7), (19, 23, 8, 7)])
def test_uv_bake_is_the_composition_and_the_restatement_bit_for_bit(shape, use_alpha):
    Th, Tw, B, Rr = shape
    s = R.synthetic_scene(Th, Tw, B, Rr, seed=Th * 1000 + Tw + B, off_coverage=True)
    t = _dev(s)
    acc, wacc = _bake(t, use_alpha)
    torch.cuda.synchronize()
    c_acc, c_wacc, p = _composition(t, use_alpha)
    assert torch.equal(acc, c_acc) and torch.equal(wacc, c_wacc), "the fused launch and the composition of uv_project + elementwise steps differ"
    d = {}
    r_acc, r_wacc = R.uv_bake(**s, use_alpha=use_alpha, detail=d)
    assert acc.cpu().numpy().tobytes() == r_acc.tobytes() and wacc.cpu().numpy().tobytes() == r_wacc.tobytes()
    e_acc, e_w = R.bake_bound(s["images"], s["wmap"], s["map_Kd"], s["weights"], use_alpha, d)      # the counted bound holds a fortiori
    assert (np.abs(acc.cpu().numpy().astype(np.float64) - r_acc) <= e_acc).all() and (np.abs(wacc.cpu().numpy().astype(np.float64) - r_wacc) <= e_w).all()
    if Th * Tw > 30 and B >= 3:      # the scene reaches what it is for: visible texels whose uv lands off the view's coverage, and the three view counts
        ua, cov = d["uv_alpha"][..., 0] > 0, d["cov"]
        vis = (s["rast2d"][..., 3] > 0)[None] & s["face_mask"].astype(bool)[:, np.clip(s["rast2d"][..., 3].astype(int) - 1, 0, None)]
        assert (vis & ~cov).any() and (vis & cov).any()
        n = ua.sum(0)
        assert (n == 0).any() and (n == 1).any() and (n >= 2).any()


def test_uv_bake_off_coverage_texel_by_hand():
    """one visible texel whose uv lands on a pixel the view does not cover: with use_alpha it adds nothing, without it takes texel [0][0] of the view's six
    channels (bg_kind NONE of utx_uv_project), colour and weight"""
    Rr = 4
    s = dict(rast2d=np.array([[[0.25, 0.25, 0.0, 1.0]]], np.float32), faces=np.array([[0, 1, 2]], np.int32), face_mask=np.ones((1, 1), np.uint8),
             v_ndc=np.full((1, 3, 2), 0.3, np.float32), images=np.zeros((1, 4, Rr, Rr), np.float32), wmap=np.zeros((1, Rr, Rr, 2), np.float32),
             rast_view=np.zeros((1, Rr, Rr, 4), np.float32), map_Kd=np.full((1, 1, 4), 0.5, np.float32), weights=np.array([2.0], np.float32))
    s["images"][0, :, 0, 0] = [0.1, 0.2, 0.3, 0.4]
    s["images"][0, :, 2, 2] = 9.0          # where uv = 0.3 lands: must not be read
    s["wmap"][0, 0, 0] = [-0.5, 0.25]
    t = _dev(s)
    acc, wacc = _bake(t, True)
    assert float(wacc.abs().max()) == 0.0 and float(acc.abs().max()) == 0.0
    acc, wacc = _bake(t, False)
    w = np.float32(2.0) * ((np.float32(-0.5) * np.float32(-0.5)) * (np.float32(-0.5) * np.float32(-0.5))) * np.float32(1.0) * (np.float32(1.0) - np.float32(0.25))
    assert wacc.cpu().numpy().ravel()[0] == w
    assert acc.cpu().numpy().ravel().tolist() == [np.float32(x) * w for x in (0.1, 0.2, 0.3, 0.4)]
    s["rast_view"][0, 2, 2, 3] = 1.0       # covered now: the sample is read
    acc, wacc = _bake(_dev(s), True)
    assert float(wacc.abs().max()) == 0.0 and np.isfinite(acc.cpu().numpy()).all()      # the weight maps are 0 around (2, 2)


@pytest.mark.parametrize("blending", [None, "soft", "hard"])
def test_uv_bake_epilogue_and_sentinels(blending):
    """the epilogue launch against the restatement, bit for bit, through the C ABI, every output between sentinels"""
    from unitex_amd._lib import ptr
    from unitex_amd.flux.ops import get_ctx
    from unitex_amd.texturetools import ops
    Th, Tw, B, Rr = 5, 7, 3, 7
    s = R.synthetic_scene(Th, Tw, B, Rr, seed=21)
    t = _dev(s)
    conf = dict(overlay_confidence=0.05, blending_confidence=0.2, inpainting_confidence=0.5)
    r_acc, r_wacc = R.uv_bake(**s)
    for thr in conf.values():
        assert 0 < (r_wacc > thr).sum() < r_wacc.size
    _, r_blend, r_mask = R.epilogue(r_acc, r_wacc, s["map_Kd"], s["rast2d"], conf["overlay_confidence"], blending, conf["blending_confidence"],
                                    conf["inpainting_confidence"])
    n = Th * Tw
    pad = 64
    bufs = {k: torch.full((pad + n * c + pad,), SENT, dtype=torch.float32, device="cuda") for k, c in (("acc", 4), ("wacc", 1), ("blended", 4))}
    mask = torch.full((pad + n + pad,), 77, dtype=torch.uint8, device="cuda")
    ctx = get_ctx(0)
    V = s["v_ndc"].shape[1]
    ctx.check(ctx.lib.utx_uv_bake(ctx.handle, ptr(t["rast2d"]), ptr(t["faces"]), 5, ptr(t["face_mask"]), ptr(t["v_ndc"]), V, B, Th, Tw, ptr(t["images"]), ptr(t["wmap"]),
                                  ptr(t["rast_view"]), Rr, ptr(t["map_Kd"]), ptr(t["weights"]), 1, ptr(bufs["acc"][pad:]), ptr(bufs["wacc"][pad:]), 1,
                                  conf["overlay_confidence"], ops.VERTEX_BLENDING[blending], conf["blending_confidence"], conf["inpainting_confidence"],
                                  ptr(bufs["blended"][pad:]), ptr(mask[pad:]), ctx.stream()))
    torch.cuda.synchronize()
    for k, c, ref in (("acc", 4, r_acc), ("wacc", 1, r_wacc), ("blended", 4, r_blend)):
        b = bufs[k].cpu().numpy()
        assert (b[:pad] == SENT).all() and (b[pad + n * c:] == SENT).all(), k
        assert b[pad:pad + n * c].tobytes() == ref.tobytes(), k
    m = mask.cpu().numpy()
    assert (m[:pad] == 77).all() and (m[pad + n:] == 77).all() and (m[pad:pad + n] == r_mask.ravel()).all()
    assert 0 < r_mask.sum() < (s["rast2d"][..., 3] > 0).sum()
    # -2 leaves the outputs alone: an unknown blending, a misaligned atlas raster, B = 0
    before = {k: v.clone() for k, v in bufs.items()}
    call = lambda **k: ctx.lib.utx_uv_bake(ctx.handle, k.get("rast2d", ptr(t["rast2d"])), ptr(t["faces"]), 5, ptr(t["face_mask"]), ptr(t["v_ndc"]), V, k.get("B", B), Th, Tw,
                                           ptr(t["images"]), ptr(t["wmap"]), ptr(t["rast_view"]), Rr, ptr(t["map_Kd"]), ptr(t["weights"]), 1, ptr(bufs["acc"][pad:]),
                                           ptr(bufs["wacc"][pad:]), 1, 0.05, k.get("blending", 1), 0.2, 0.5, ptr(bufs["blended"][pad:]), ptr(mask[pad:]), ctx.stream())
    assert call(blending=3) == -2 and call(rast2d=t["rast2d"].data_ptr() + 4) == -2 and call(B=0) == -2
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], bufs[k]) for k in bufs)


def _hand_masks():
    corner = np.zeros((9, 9), np.uint8)
    corner[0, 0] = 1
    border = np.ones((6, 5), np.uint8)
    border[3, 2] = 0
    return corner, border


@pytest.mark.parametrize("C", [1, 3, 4, 16])
def test_uv_dilation_is_the_restatement_bit_for_bit(C):
    from unitex_amd.texturetools import ops
    rng = np.random.default_rng(C)
    corner, border = _hand_masks()
    cases = [("one valid corner texel in 9 x 9", corner, 8), ("all valid", np.ones((4, 6), np.uint8), 0), ("none valid", np.zeros((4, 6), np.uint8), 1),
             ("a valid border texel re-averaged", border, 1), ("H = 1", (rng.uniform(0, 1, (1, 37)) < 0.3).astype(np.uint8), None),
             ("W = 1", (rng.uniform(0, 1, (41, 1)) < 0.3).astype(np.uint8), None), ("more than one block", (rng.uniform(0, 1, (33, 29)) < 0.05).astype(np.uint8), None)]
    for name, valid, steps in cases:
        if valid.max() == 0 and steps is None:
            valid[0, 0] = 1
        col = rng.uniform(-0.5, 1.5, valid.shape + (C,)).astype(np.float32)      # values outside [0, 1]
        trace_r, trace_g = [], []
        ref, n_ref = R.uv_dilation(col, valid, trace=trace_r)
        got, n = ops.uv_dilation(torch.from_numpy(col).cuda(), torch.from_numpy(valid).cuda(), trace=trace_g)
        assert n == n_ref and (steps is None or n == steps), (name, n, n_ref, steps)
        for k, ((rc, rm), (gc, gm)) in enumerate(zip(trace_r, trace_g)):
            assert gc.cpu().numpy().tobytes() == rc.tobytes() and (gm.cpu().numpy() == rm).all(), "%s: step %d" % (name, k)
        assert got.cpu().numpy().tobytes() == ref.tobytes(), name
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
        if name == "none valid":
            assert got.cpu().numpy().tobytes() == R.clamp01(col).tobytes()
        if name == "a valid border texel re-averaged":      # the valid corner (0, 0) has out-of-image neighbours: M = 4, not 9
            assert trace_r[0][0][0, 0].tobytes() != col[0, 0].tobytes()
    # max_iters stops the loop; the texels out of reach keep their (clamped) colour
    col = rng.uniform(0, 1, (9, 9, C)).astype(np.float32)
    got, n = ops.uv_dilation(torch.from_numpy(col).cuda(), torch.from_numpy(corner).cuda(), max_iters=2)
    ref, n_ref = R.uv_dilation(col, corner, max_iters=2)
    assert n == n_ref == 2 and got.cpu().numpy().tobytes() == ref.tobytes() and (got.cpu().numpy()[5:, 5:] == col[5:, 5:]).all()


def test_uv_dilation_step_abi_sentinels_and_counter():
    from unitex_amd._lib import ptr
    from unitex_amd.flux.ops import get_ctx
    ctx = get_ctx(0)
    H, W, C, pad = 5, 7, 3, 64
    rng = np.random.default_rng(5)
    col = rng.uniform(0, 1, (H, W, C)).astype(np.float32)
    valid = np.zeros((H, W), np.uint8)
    valid[2, 3] = 1
    r_col, r_mask, r_left = R.dilation_step(col, valid)
    out = torch.full((pad + H * W * C + pad,), SENT, dtype=torch.float32, device="cuda")
    mo = torch.full((pad + H * W + pad,), 77, dtype=torch.uint8, device="cuda")
    cnt = torch.full((3,), -5, dtype=torch.int32, device="cuda")
    ci, mi = torch.from_numpy(col).cuda(), torch.from_numpy(valid).cuda()
    step = ctx.lib.utx_uv_dilation_step
    ctx.check(step(ctx.handle, ptr(ci), ptr(mi), H, W, C, 0, ptr(out[pad:]), ptr(mo[pad:]), ptr(cnt[1:]), ctx.stream()))
    torch.cuda.synchronize()
    o, m = out.cpu().numpy(), mo.cpu().numpy()
    assert (o[:pad] == SENT).all() and (o[pad + H * W * C:] == SENT).all() and o[pad:pad + H * W * C].tobytes() == r_col.tobytes()
    assert (m[:pad] == 77).all() and (m[pad + H * W:] == 77).all() and (m[pad:pad + H * W] == r_mask.ravel()).all()
    assert cnt.cpu().tolist() == [-5, r_left, -5] and r_left == H * W - 9
    before = out.clone()
    assert step(ctx.handle, ptr(ci), ptr(mi), H, W, 17, 0, ptr(out[pad:]), ptr(mo[pad:]), ptr(cnt[1:]), ctx.stream()) == -2
    assert step(ctx.handle, ptr(ci), ptr(mi), H, W, C, 2, ptr(out[pad:]), ptr(mo[pad:]), ptr(cnt[1:]), ctx.stream()) == -2
    assert step(ctx.handle, ptr(ci), ptr(mi), H, W, C, 0, ptr(ci), ptr(mo[pad:]), ptr(cnt[1:]), ctx.stream()) == -2
    assert step(ctx.handle, ptr(ci), ptr(mi), H, W, C, 0, ptr(out[pad:]), ptr(mi), ptr(cnt[1:]), ctx.stream()) == -2
    assert step(ctx.handle, ptr(ci), ptr(mi), 0, W, C, 0, ptr(out[pad:]), ptr(mo[pad:]), ptr(cnt[1:]), ctx.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(before, out) and cnt.cpu().tolist() == [-5, r_left, -5]


# ---- the public functions against the reference's own arrays (fixture G21)
def _g21_mesh():
    from unitex_amd.texturetools.renderer_inverse import DeviceMesh
    f = R.g21()
    return f, DeviceMesh(f["verts"], f["faces"], f["uvs"], "cuda").set_vertex_normals(f["v_nrm"])


@pytest.mark.parametrize("tag,perspective", [("p", True), ("o", False)])
def test_remapping_uv_texture_against_g21(tag, perspective):
    from unitex_amd.texturetools import remapping_uv as RU
    f, mesh = _g21_mesh()
    Rs, T = int(f["render_size"]), int(f["texture_size"])
    conf = dict(zip(("overlay_confidence", "blending_confidence", "inpainting_confidence"), [float(x) for x in f["conf"]]))
    c2ws, intr, images, kd, w3 = f["c2ws_" + tag], f["intr_" + tag], R.g21_images()[:3], R.g21_map_Kd(), f["weights3"]
    cmax = max(float(np.abs(kd).max()), float(np.abs(images).max()), 1.0)
    worst = {}
    for ua in (True, False):
        acc, wacc = RU.project_uv_texture(mesh, c2ws, intr, images, kd, w3, use_alpha=ua, render_size=Rs, texture_size=T, perspective=perspective)
        r_acc, r_wacc = f["acc_%s_a%d" % (tag, ua)], f["wacc_%s_a%d" % (tag, ua)]
        # the bound is evaluated on the reference's own per-view arrays, stored in the fixture
        d = {}
        R.uv_bake(**R.g21_inputs(tag), use_alpha=ua, detail=d)      # the restatement on the reference's own inputs: the magnitudes the bound is counted on
        e_acc, e_w = R.bake_bound(images, f["wmap_" + tag], kd, w3, ua, d)
        da, dw = np.abs(acc.cpu().numpy().astype(np.float64) - r_acc), np.abs(wacc.cpu().numpy().astype(np.float64) - r_wacc)
        worst["acc a%d" % ua] = (da.max() / U, e_acc.max() / U)
        print("G21 %s use_alpha=%d: acc off by at most %.2f u (bound up to %.1f u), wacc %.2f u (%.1f u)" % (tag, ua, da.max() / U, e_acc.max() / U, dw.max() / U, e_w.max() / U))
        assert (da <= e_acc).all() and (dw <= e_w).all()
    d = {}
    R.uv_bake(**R.g21_inputs(tag), use_alpha=True, detail=d)
    e_acc, e_w = R.bake_bound(images, f["wmap_" + tag], kd, w3, True, d)
    for blending in ("soft", "hard"):
        out, st = RU.remapping_uv_texture(mesh, c2ws, intr, images, map_Kd=kd, weights=list(w3), blending_type=blending, use_cv_inpainting=False, render_size=Rs,
                                          texture_size=T, perspective=perspective, return_stages=True, **conf)
        e_b = R.epilogue_bound(f["acc_%s_a1" % tag], f["wacc_%s_a1" % tag], kd, e_acc, e_w, conf["overlay_confidence"], blending, conf["blending_confidence"])
        ref_b = f["blended_%s_%s" % (blending, tag)]
        db = np.abs(st["blended"].cpu().numpy()[..., :3].astype(np.float64) - ref_b[..., :3])
        assert (db <= e_b[..., :3]).all(), "blended %s: %.2f u" % (blending, db.max() / U)
        assert (st["inpaint_mask"].cpu().numpy() == f["inpaint_mask_" + tag]).all()
        if blending == "hard":      # the fixture stores the later stages for 'soft' only
            continue
        assert st["inpaint_steps"] == int(f["steps_%s_%s" % (blending, tag)])
        e_in = R.dilation_bound(float(e_b[..., :3].max()), st["inpaint_steps"], cmax)
        di = np.abs(st["inpainted"].cpu().numpy().astype(np.float64) - f["inpainted_%s_%s" % (blending, tag)])
        assert di.max() <= e_in, "inpainted %s: %.2f u over %.2f u" % (blending, di.max() / U, e_in / U)
        e_out = R.outpaint_bound(e_in, T, cmax)
        ref = f["final_%s_%s" % (blending, tag)]
        do = np.abs(out.cpu().numpy().astype(np.float64) - ref)
        print("G21 %s %s: blended %.2f u (bound up to %.1f u), inpainted %.2f u (%.1f u), final %.2f u (%.1f u), %d steps" % (
            tag, blending, db.max() / U, e_b[..., :3].max() / U, di.max() / U, e_in / U, do.max() / U, e_out / U, st["inpaint_steps"]))
        assert do.max() <= e_out and (out.cpu().numpy()[..., 3] == ref[..., 3]).all()
        # return_stages agrees with the separate calls
        plain = RU.remapping_uv_texture(mesh, c2ws, intr, images, map_Kd=kd, weights=list(w3), blending_type=blending, use_cv_inpainting=False, render_size=Rs,
                                        texture_size=T, perspective=perspective, **conf)
        assert torch.equal(plain, out) and torch.equal(st["map_Kd"], out)
    acc, wacc = RU.project_uv_texture(mesh, c2ws, intr, images, kd, w3, render_size=Rs, texture_size=T, perspective=perspective)
    assert torch.equal(acc, st["map_Kd_rgb_acc"]) and torch.equal(wacc, st["map_Kd_weight_acc"])
    filled = RU.uv_dilation(st["blended"][..., :3].permute(2, 0, 1)[None], st["inpaint_mask"][None, None])
    assert torch.equal(filled[0].permute(1, 2, 0), st["inpainted"])


def test_remapping_uv_texture_six_views_default_weights_and_none_map():
    from unitex_amd.texturetools import remapping_uv as RU
    f, mesh = _g21_mesh()
    Rs, T = int(f["render_size"]), int(f["texture_size"])
    out, st = RU.remapping_uv_texture(mesh, f["c2ws_6"], f["intr_6"], R.g21_images(), map_Kd=R.g21_map_Kd(), use_cv_inpainting=False, use_inpainting=False,
                                      use_outpainting=False, render_size=Rs, texture_size=T, return_stages=True)
    ref = f["final_6"]
    d = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    # six views of the default weight table through the overlay and the soft blending at the default confidences (0.2)
    d6, s6 = {}, R.g21_inputs("6")
    R.uv_bake(**s6, use_alpha=True, detail=d6)
    e_acc, e_w = R.bake_bound(s6["images"], s6["wmap"], s6["map_Kd"], s6["weights"], True, d6)
    e_b = R.epilogue_bound(f["acc_6"], f["wacc_6"], s6["map_Kd"], e_acc, e_w, 0.2, "soft", 0.2)
    print("G21 six views: final off by at most %.2f u (bound up to %.1f u)" % (d[..., :3].max() / U, e_b[..., :3].max() / U))
    assert (d[..., :3] <= e_b[..., :3]).all() and (out.cpu().numpy()[..., 3] == ref[..., 3]).all()
    assert str(f["map_kd_none"]).startswith("RuntimeError")      # reading (a): the reference cannot run map_Kd=None
    none = RU.remapping_uv_texture(mesh, f["c2ws_p"], f["intr_p"], R.g21_images()[:3], map_Kd=None, use_cv_inpainting=False, render_size=Rs, texture_size=T)
    zero = RU.remapping_uv_texture(mesh, f["c2ws_p"], f["intr_p"], R.g21_images()[:3], map_Kd=np.zeros((T, T, 3), np.float32), use_blending=False,
                                   use_cv_inpainting=False, render_size=Rs, texture_size=T)
    assert torch.equal(none, zero) and tuple(none.shape) == (T, T, 4)
