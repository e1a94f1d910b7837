"""Telea inpainting on the GPU: utx_inpaint_distance / utx_inpaint_telea_step / utx_inpaint_finish through ops.inpaint_distance and ops.inpaint_telea against
the float64 restatement of the rule (tests/support/inpaint_ref.py) with the per-case bound 4 d measured on the CPU (tests/test_inpaint_cpu.py), and
uv_dilation_cv / image_outpainting / remapping_uv_texture_cv against the composition of their stages.

Measured on the first MI355X run: the float output equals the float32 restatement BIT FOR BIT on every case (0 uint8 steps of difference), so the product's own
difference from the float64 restatement is d itself."""
import numpy as np
import pytest
import torch

from oracle import uv_bake_ref as G
from tests.support import inpaint_ref as R

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in R.cases()]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unit(u8):
    """a uint8 result as the wrappers hand it back: float32 / 255, by the device's own division"""
    return _cuda(u8).to(torch.float32).div(255)


@pytest.mark.parametrize("name", NAMES)
def test_inpaint_distance_is_the_brute_force_bit_for_bit(name):
    from unitex_amd.texturetools import ops
    hole = R.reference(name)["hole"]
    got = ops.inpaint_distance(_cuda(hole)).cpu().numpy()
    assert got.dtype == np.int32 and got.tobytes() == R.distance_brute(hole).tobytes()
    got = ops.inpaint_distance(_cuda(hole * 255)).cpu().numpy()      # any non-zero value is a hole
    assert got.tobytes() == R.distance_brute(hole).tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_inpaint_telea_against_the_float64_restatement(name):
    from unitex_amd.texturetools import ops
    c = R.reference(name)
    img, hole = _cuda(c["img"]), _cuda(c["hole"])
    u, f, sweeps = ops.inpaint_telea(img, hole, radius=c["eps"], return_float=True, readback=1)
    u, f = u.cpu().numpy(), f.cpu().numpy()
    d64 = float(np.abs(f.astype(np.float64) - c["f64"]).max())
    d32 = float(np.abs(f.astype(np.float64) - c["f32"].astype(np.float64)).max())
    print("%s: %d sweeps, |gpu - float64| = %.3g, |gpu - float32 restatement| = %.3g uint8 steps (d = %.3g, bound %.3g)" % (name, sweeps, d64, d32, c["d"], c["bound"]))
    bad = R.compare(u, f, c["f64"], c["hole"], c["bound"])
    assert not bad, bad
    assert (u[c["hole"] == 0] == c["img"][c["hole"] == 0]).all()      # the pixels outside the hole are kept
    # the same operations in the same order without contraction, with correctly rounded division and square root: the float32 restatement's bits
    assert f.tobytes() == c["f32"].tobytes() and u.tobytes() == c["u32"].tobytes()
    # read back after every sweep, the loop stops with the longest dependency chain, which the restatement's sweep schedule counts
    assert sweeps == R.telea(c["img"], c["hole"], c["eps"], np.float32, schedule="sweep")[2]
    # a second run, and a run that reads the counter back every 4 sweeps, give the same bytes
    u2, f2, s2 = ops.inpaint_telea(img, hole, radius=c["eps"], return_float=True, readback=1)
    u4, f4, s4 = ops.inpaint_telea(img, hole, radius=c["eps"], return_float=True, readback=4)
    assert u2.cpu().numpy().tobytes() == u.tobytes() and f2.cpu().numpy().tobytes() == f.tobytes() and s2 == sweeps
    assert u4.cpu().numpy().tobytes() == u.tobytes() and f4.cpu().numpy().tobytes() == f.tobytes() and s4 == -(-sweeps // 4) * 4
    if sweeps == 0:
        assert u.tobytes() == c["img"].tobytes()


def test_inpaint_telea_edges_of_the_wrapper():
    from unitex_amd.texturetools import ops
    c = R.reference("33x31 two holes closer than 2 eps, eps 2")
    img, hole = _cuda(c["img"]), _cuda(c["hole"])
    out, sweeps = ops.inpaint_telea(img, hole, radius=2)
    assert out.cpu().numpy().tobytes() == c["u32"].tobytes() and out.dtype == torch.uint8
    one = R.telea(c["img"], c["hole"], 1, np.float32)[0]
    for radius in (1, 0, -1):      # OpenCV clamps the reference's -1 to 1
        assert ops.inpaint_telea(img, hole, radius=radius)[0].cpu().numpy().tobytes() == one.tobytes()
    trace = []
    ops.inpaint_telea(img, hole, radius=2, trace=trace, readback=1)
    assert len(trace) == 3 and int(trace[-1].min()) == 1 and int(trace[0].min()) == 0
    e = torch.zeros(0, 5, 3, dtype=torch.uint8, device="cuda")
    out, sweeps = ops.inpaint_telea(e, torch.zeros(0, 5, dtype=torch.uint8, device="cuda"))
    assert tuple(out.shape) == (0, 5, 3) and sweeps == 0
    assert tuple(ops.inpaint_distance(torch.zeros(0, 5, dtype=torch.uint8, device="cuda")).shape) == (0, 5)
    assert int(ops.inpaint_distance(torch.ones(3, 4, dtype=torch.uint8, device="cuda")).min()) == R.NONE


def test_step_abi_sentinels_counter_and_refusals():
    from unitex_amd._lib import ptr
    from unitex_amd.flux.ops import get_ctx
    from unitex_amd.texturetools import ops
    ctx = get_ctx(0)
    c = R.reference("5x7 ring on every border and corner")
    H, W, C, pad, SENT = 5, 7, 3, 64, 12345.0
    hole = _cuda(c["hole"])
    d2 = ops.inpaint_distance(hole)
    col = _cuda(c["img"]).to(torch.float32).contiguous()
    done = (hole == 0).to(torch.uint8)
    out = torch.full((pad + H * W * C + pad,), SENT, dtype=torch.float32, device="cuda")
    out[pad:pad + H * W * C] = col.reshape(-1)      # both buffers hold the image outside the hole
    dn = torch.full((pad + H * W + pad,), 77, dtype=torch.uint8, device="cuda")
    dn[pad:pad + H * W] = done.reshape(-1)
    cnt = torch.tensor([-5, 100, -5], dtype=torch.int32, device="cuda")
    step = ctx.lib.utx_inpaint_telea_step
    ctx.check(step(ctx.handle, ptr(col), ptr(done), ptr(d2), H, W, C, 3, ptr(out[pad:]), ptr(dn[pad:]), ptr(cnt[1:]), ctx.stream()))
    torch.cuda.synchronize()
    first = int((c["hole"] != 0).sum() - (R.distance(c["hole"]) > 1).sum())      # every pixel at distance 1 is ready at once
    o, m = out.cpu().numpy(), dn.cpu().numpy()
    assert (o[:pad] == SENT).all() and (o[pad + H * W * C:] == SENT).all() and (m[:pad] == 77).all() and (m[pad + H * W:] == 77).all()
    assert cnt.cpu().tolist() == [-5, 100 + first, -5]      # the counter is increased, not zeroed
    assert int(m[pad:pad + H * W].sum()) == int((c["hole"] == 0).sum()) + first
    before, before_d = out.clone(), dn.clone()
    call = lambda **k: step(ctx.handle, k.get("col_in", ptr(col)), ptr(done), ptr(d2), H, W, k.get("C", C), k.get("radius", 3), ptr(out[pad:]),
                            k.get("done_out", ptr(dn[pad:])), ptr(cnt[1:]), ctx.stream())
    assert call(C=5) == -2 and call(radius=0) == -2 and call(radius=9) == -2 and call(col_in=ptr(out[pad:])) == -2 and call(done_out=ptr(done)) == -2
    assert ctx.lib.utx_inpaint_finish(ctx.handle, ptr(col), H, W, 5, ptr(dn[pad:]), None, ctx.stream()) == -2
    torch.cuda.synchronize()
    assert torch.equal(before, out) and torch.equal(before_d, dn) and cnt.cpu().tolist() == [-5, 100 + first, -5]


def test_uv_dilation_cv_batch_and_image_outpainting():
    from unitex_amd.texturetools import ops, remapping_uv as RU
    from unitex_amd.texturetools.image_outpainting import image_outpainting
    rng = np.random.default_rng(8)
    kd = torch.from_numpy(rng.uniform(-0.2, 1.2, (3, 3, 33, 31)).astype(np.float32)).cuda()      # values outside [0, 1]: the quantisation clamps
    mask = torch.from_numpy(rng.uniform(0, 1, (3, 1, 33, 31)) < 0.3).cuda()
    keep = kd.clone()
    got = RU.uv_dilation_cv(kd, mask)
    assert torch.equal(kd, keep) and got.dtype == kd.dtype and tuple(got.shape) == tuple(kd.shape)
    for i in range(3):      # every image of the batch is filled on its own
        assert torch.equal(got[i:i + 1], RU.uv_dilation_cv(kd[i:i + 1], mask[i:i + 1]))
        q = (kd[i].permute(1, 2, 0).clamp(0, 1) * 255).to(torch.uint8)
        ref = R.telea(q.cpu().numpy(), mask[i, 0].cpu().numpy(), 1, np.float32)[0]      # max_iters = -1 is the radius, clamped to 1
        assert torch.equal(got[i].permute(1, 2, 0), _unit(ref))
    r3 = RU.uv_dilation_cv(kd[:1], mask[:1], max_iters=3)
    q = (kd[0].permute(1, 2, 0).clamp(0, 1) * 255).to(torch.uint8)
    assert torch.equal(r3[0].permute(1, 2, 0), _unit(R.telea(q.cpu().numpy(), mask[0, 0].cpu().numpy(), 3, np.float32)[0]))
    # image_outpainting(method='telea'): the reference's hand-off, the mask resized by n_erode_pix
    src = kd.permute(0, 2, 3, 1).contiguous()
    m = torch.zeros(1, 33, 31, 1, device="cuda")
    m[0, 10:20, 8:22] = 1.0
    for n in (0, 3, -3):
        out = image_outpainting(src, m, n_erode_pix=n, n_radius=2, method="telea")
        mm = ops.mask_morph((m[0, :, :, 0] * 255).to(torch.uint8).contiguous(), n)
        assert tuple(out.shape) == (3, 33, 31, 3)
        for i in range(3):
            q = (src[i].clamp(0, 1) * 255).to(torch.uint8).contiguous()
            assert torch.equal(out[i], ops.inpaint_telea(q, mm, radius=2)[0].to(torch.float32) / 255.0)
    with pytest.raises(NotImplementedError, match="'telea'"):
        image_outpainting(src, m)


def _g21_mesh():
    from unitex_amd.texturetools.renderer_inverse import DeviceMesh
    f = G.g21()
    return f, DeviceMesh(f["verts"], f["faces"], f["uvs"], "cuda").set_vertex_normals(f["v_nrm"])


@pytest.mark.parametrize("T,Rs", [(19, 7), (32, 8)])
def test_remapping_uv_texture_cv_is_the_composition_of_its_stages(T, Rs):
    """the small scene of the blended bake's tests (the G21 mesh, three views) at a 19 x 19 and a 32 x 32 atlas"""
    from unitex_amd.texturetools import ops, remapping_uv as RU
    from unitex_amd.texturetools.image_fusion import image_fusion
    f, mesh = _g21_mesh()
    rng = np.random.default_rng(T)
    images = rng.uniform(0, 1, (3, 4, Rs, Rs)).astype(np.float32)
    kd = rng.uniform(0, 1, (T, T, 4)).astype(np.float32)
    conf = dict(overlay_confidence=0.05, blending_confidence=0.2, inpainting_confidence=0.5)
    kw = dict(map_Kd=kd, weights=list(f["weights3"]), render_size=Rs, texture_size=T, **conf)
    args = (mesh, f["c2ws_p"], f["intr_p"], images)
    # the cv flags off: remapping_uv_texture's bytes
    for blending in ("soft", "hard"):
        a = RU.remapping_uv_texture(*args, blending_type=blending, use_cv_inpainting=False, **kw)
        b = RU.remapping_uv_texture_cv(*args, blending_type=blending, use_cv_inpainting=False, **kw)
        assert torch.equal(a, b)
    # the defaults (use_cv_inpainting=True, the reference's own call): stages + uv_dilation_cv + pull_push
    out, st = RU.remapping_uv_texture_cv(*args, return_stages=True, **kw)
    mask, covered = st["inpaint_mask"], out[..., 3].to(torch.uint8).contiguous()
    print("T = %d: %d texels to inpaint, %d of %d covered" % (T, int(mask.sum()), int(covered.sum()), T * T))
    assert 0 < int(mask.sum()) and 0 < int(covered.sum()) < T * T
    rgb = RU.uv_dilation_cv(st["blended"][..., :3].permute(2, 0, 1)[None], mask[None, None] != 0)[0].permute(1, 2, 0).contiguous()
    assert torch.equal(rgb, st["inpainted"]) and st["inpaint_steps"] == 0
    assert torch.equal(out[..., :3], ops.pull_push(rgb, covered))
    assert torch.equal(out, RU.remapping_uv_texture_cv(*args, **kw))
    soft = RU.remapping_uv_texture(*args, use_cv_inpainting=False, return_stages=True, **kw)[1]
    assert torch.equal(soft["blended"], st["blended"]) and torch.equal(soft["inpaint_mask"], mask)
    q = (st["blended"][..., :3].clamp(0, 1) * 255).to(torch.uint8)
    ref = R.telea(q.cpu().numpy(), mask.cpu().numpy(), 1, np.float32)[0]
    assert torch.equal(st["inpainted"], _unit(ref))
    # use_cv_outpainting=True: the texels the atlas does not cover go through uv_dilation_cv as well
    out2 = RU.remapping_uv_texture_cv(*args, use_cv_outpainting=True, **kw)
    assert torch.equal(out2[..., :3], RU.uv_dilation_cv(rgb.permute(2, 0, 1)[None], (covered == 0)[None, None])[0].permute(1, 2, 0))
    assert torch.equal(out2[..., 3], out[..., 3])
    # 'poisson': the overlay stage (a bake with no blending in the epilogue) through image_fusion
    outp, stp = RU.remapping_uv_texture_cv(*args, blending_type="poisson", return_stages=True, **kw)
    acc, wacc = RU.project_uv_texture(*args, torch.from_numpy(kd).cuda(), f["weights3"], render_size=Rs, texture_size=T)
    overlay = torch.where(wacc > conf["overlay_confidence"], acc / wacc, acc)
    none = RU.remapping_uv_texture(*args, use_blending=False, use_cv_inpainting=False, return_stages=True, **kw)[1]
    assert torch.equal(none["blended"], overlay)
    fused = image_fusion(overlay[None, ..., :3], torch.from_numpy(kd).cuda()[None, ..., :3], (wacc > conf["blending_confidence"]).float()[None])[0]
    assert torch.equal(stp["blended"][..., :3], fused) and torch.equal(stp["inpaint_mask"], mask)
    rgbp = RU.uv_dilation_cv(fused.permute(2, 0, 1)[None], mask[None, None] != 0)[0].permute(1, 2, 0).contiguous()
    assert torch.equal(outp[..., :3], ops.pull_push(rgbp, covered))
