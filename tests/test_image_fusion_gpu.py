"""Poisson image fusion on the GPU (csrc/image_fusion.hip: utx_mask_morph, utx_mask_bbox, utx_image_fusion) through the C ABI and the Python surface
(ops.mask_morph, ops.mask_bbox, ops.image_fusion_u8, texturetools.image_fusion), against the float64 restatement with its exact sine-transform solve
(tests/support/image_fusion_ref.py).

Acceptance (R.compare): d = max |float32 output - float64 oracle| in uint8 units <= BOUND = 4 x the value recorded on the MI355X, never above 0.25; every
uint8 output within one step of the oracle's rounding and equal to it wherever the oracle's unrounded value is farther than BOUND from a rounding tie and from the
clamp edges; the share excused that way, counted from the oracle alone, at most 2 BOUND + 1 %; the uint8 output is the half-even rounding of the float output;
everything outside the rectangle's interior is dst, byte for byte; two calls give the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.support import image_fusion_ref as R

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda().contiguous()


@pytest.fixture(scope="module")
def ops():
    from unitex_amd.texturetools import ops
    return ops


def _check(ops, name, case):
    ref = R.fuse(case["src"], case["dst"], case["mask"], case["n"])
    src, dst, mask = _cuda(case["src"]), _cuda(case["dst"]), _cuda(case["mask"])
    out, out_f = ops.image_fusion_u8(src, dst, mask, n_erode_pix=case["n"], return_float=True)
    again, again_f = ops.image_fusion_u8(src, dst, mask, n_erode_pix=case["n"], return_float=True)
    assert torch.equal(out, again) and torch.equal(out_f, again_f), "two calls differ"
    assert torch.equal(ops.image_fusion_u8(src, dst, mask, n_erode_pix=case["n"]), out)
    if case["n"]:
        m = ops.mask_morph(mask, case["n"])
        assert np.array_equal(m.cpu().numpy(), ref["mask"])
        assert ops.mask_bbox(m) == ref["rect"]
    else:
        assert ops.mask_bbox(mask) == ref["rect"]
    problems, d, share = R.compare(out.cpu().numpy(), out_f.cpu().numpy(), case["dst"], ref)
    print("%-28s rect %-22s d = %.3g (bound %.3g), excused %.4f" % (name, ref["rect"], d, R.BOUND, share))
    assert not problems, (name, problems)


@pytest.mark.parametrize("name", list(R.edge_cases()))
def test_edge_shapes_against_the_float64_oracle(ops, name):
    _check(ops, name, R.edge_cases()[name])


def test_scale_1024_disc_of_radius_400(ops):
    _check(ops, "scale_1024", R.scale_case())


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 31, -1, -2, -4, -7, -31])
def test_mask_morph_matches_the_restatement(ops, n):
    rng = np.random.default_rng(abs(n))
    H, W = 70, 131      # more than one block, no multiple of it
    mask = np.maximum(R.ellipse_mask(H, W, 0, 2, 60, 41), R.box_mask(H, W, 100, 50, 31, 20))
    mask[rng.integers(0, H, 40), rng.integers(0, W, 40)] = rng.integers(0, 255, 40)
    got = ops.mask_morph(_cuda(mask), n)
    assert np.array_equal(got.cpu().numpy(), R.morph(mask, n))
    assert ops.mask_bbox(got) == R.bounding_rect(R.morph(mask, n))


def test_bounding_rectangle_of_single_pixels_and_of_nothing(ops):
    H, W = 257, 300
    assert ops.mask_bbox(torch.zeros(H, W, dtype=torch.uint8, device="cuda")) == (0, 0, 0, 0)
    for y, x in ((0, 0), (256, 299), (100, 7)):
        m = torch.zeros(H, W, dtype=torch.uint8, device="cuda")
        m[y, x] = 1
        assert ops.mask_bbox(m) == (x, y, 1, 1)


def _float_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.rand(B, H, W, 3, generator=g) * 1.2 - 0.1      # values outside [0, 1] are clamped
    dst = torch.rand(1, H, W, 3, generator=g)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = torch.as_tensor((((xx - 30) / 21.0) ** 2 + ((yy - 24) / 15.0) ** 2 <= 1.0).astype(np.float32))[None, ..., None]
    return src, dst, mask


def _quantise(t):
    return (np.clip(t.numpy().astype(np.float32), 0.0, 1.0) * np.float32(255)).astype(np.uint8)


def test_image_fusion_on_floats_is_the_uint8_path_through_the_quantisation(ops):
    """B = 2 with dst and the mask broadcast over the batch"""
    from unitex_amd.texturetools.image_fusion import image_fusion
    src, dst, mask = _float_inputs(2, 50, 64, 7)
    got = image_fusion(src.cuda(), dst.cuda(), mask.cuda(), n_erode_pix=-1)
    assert got.shape == (2, 50, 64, 3) and got.dtype == torch.float32
    for i in range(2):
        s, d, m = _quantise(src[i]), _quantise(dst[0]), _quantise(mask[0, :, :, 0])
        want = ops.image_fusion_u8(_cuda(s), _cuda(d), _cuda(m), n_erode_pix=-1)
        assert torch.equal(got[i], want.to(torch.float32).div(255.0))
        ref = R.fuse(s, d, m, -1)
        problems, dd, share = R.compare(want.cpu().numpy(), ops.image_fusion_u8(_cuda(s), _cuda(d), _cuda(m), n_erode_pix=-1, return_float=True)[1].cpu().numpy(), d, ref)
        print("batch %d: d = %.3g, excused %.4f" % (i, dd, share))
        assert not problems, problems
    half = image_fusion(src.cuda().half(), dst.cuda().half(), mask.cuda().half())
    assert half.dtype == torch.float16 and half.shape == got.shape


def test_image_fusion_hybrid_is_the_pre_blend_and_the_fusion(ops):
    from unitex_amd.texturetools.image_fusion import image_fusion_hybrid
    src, dst, mask = _float_inputs(1, 50, 64, 8)
    mask = mask * 0.75 + 0.25 * (mask > 0) * torch.rand(mask.shape, generator=torch.Generator().manual_seed(9))      # grey values: the pre-blend weighs by them
    yy, xx = np.mgrid[0:50, 0:64]
    boundary = torch.as_tensor(((np.abs(xx - 30) < 6) * 0.8).astype(np.float32))[None, ..., None]
    n = 3
    got = image_fusion_hybrid(src.cuda(), dst.cuda(), mask.cuda(), boundary.cuda(), n_erode_pix=n)
    s, d, m0, b = _quantise(src[0]), _quantise(dst[0]), _quantise(mask[0, :, :, 0]), _quantise(boundary[0, :, :, 0])
    m = R.morph(m0, n)
    mb = b * (m > 127)
    mf, bf = (m / 255.0)[..., None], (mb / 255.0)[..., None]
    d2 = np.clip((s * mf + d * (1.0 - mf)) * bf + d * (1.0 - bf), 0.0, 255.0).astype(np.uint8)
    assert (d2 != d).any()
    want = ops.image_fusion_u8(_cuda(s), _cuda(d2), _cuda(m))
    assert torch.equal(got[0], want.to(torch.float32).div(255.0))
    ref = R.fuse(s, d2, m)
    problems, dd, share = R.compare(want.cpu().numpy(), ops.image_fusion_u8(_cuda(s), _cuda(d2), _cuda(m), return_float=True)[1].cpu().numpy(), d2, ref)
    print("hybrid: d = %.3g, excused %.4f" % (dd, share))
    assert not problems, problems


def test_c_abi_misuse_leaves_the_outputs_alone(ops):
    from unitex_amd._lib import ptr
    from unitex_amd.flux.ops import get_ctx
    ctx = get_ctx(torch.cuda.current_device())
    lib, h, st = ctx.lib, ctx.handle, ctx.stream()
    H, W = 20, 24
    img = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda")
    mask = torch.full((H, W), 255, dtype=torch.uint8, device="cuda")
    out = torch.full((H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
    out_f = torch.full((H, W, 3), -77.0, device="cuda")
    need = lib.utx_image_fusion_workspace_bytes(W, H)
    work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    def fuse(src=img, dst=img, m=mask, HH=H, WW=W, rect=(0, 0, W, H), cycles=0, o=out, wk=work, nbytes=need):
        return lib.utx_image_fusion(h, ptr(src), ptr(dst), ptr(m), HH, WW, *rect, cycles, ptr(o), ptr(out_f), ptr(wk), nbytes, st)
    assert fuse(src=None) == -2 and fuse(dst=None) == -2 and fuse(m=None) == -2 and fuse(o=None) == -2 and fuse(wk=None) == -2
    assert fuse(HH=0) == -2 and fuse(WW=0) == -2 and fuse(rect=(0, 0, W + 1, H)) == -2 and fuse(rect=(-1, 0, 4, 4)) == -2 and fuse(rect=(3, 18, 4, 3)) == -2
    assert fuse(nbytes=need - 1) == -2 and fuse(cycles=-1) == -2 and fuse(cycles=65) == -2
    tmp, mo = torch.full((H, W), 0xCD, dtype=torch.uint8, device="cuda"), torch.full((H, W), 0xEF, dtype=torch.uint8, device="cuda")
    morph = lambda mi=mask, HH=H, WW=W, n=3, t=tmp, o=mo: lib.utx_mask_morph(h, ptr(mi), HH, WW, n, ptr(t), ptr(o), st)
    assert morph(mi=None) == -2 and morph(t=None) == -2 and morph(o=None) == -2 and morph(HH=0) == -2 and morph(WW=0) == -2
    assert morph(n=0) == -2 and morph(n=32) == -2 and morph(n=-32) == -2 and morph(t=mask) == -2 and morph(t=mo) == -2
    rect = torch.full((4,), 123, dtype=torch.int32, device="cuda")
    assert lib.utx_mask_bbox(h, None, H, W, ptr(rect), st) == -2 and lib.utx_mask_bbox(h, ptr(mask), H, W, None, st) == -2 and lib.utx_mask_bbox(h, ptr(mask), 0, W, ptr(rect), st) == -2
    torch.cuda.synchronize()
    assert (out == 0xAB).all() and (out_f == -77.0).all() and (tmp == 0xCD).all() and (mo == 0xEF).all() and (rect == 123).all()
    # and the calls that are right go through: no interior needs no workspace
    assert lib.utx_image_fusion(h, ptr(img), ptr(img), ptr(mask), H, W, 2, 3, 9, 2, 0, ptr(out), None, None, 0, st) == 0
    assert fuse() == 0 and morph() == 0
    torch.cuda.synchronize()
    assert (out == 7).all() and (out_f == 7.0).all() and (mo == 255).all()
