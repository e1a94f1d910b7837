"""Telea inpainting (unitex_amd/csrc/inpaint.hip, ops.inpaint_telea, remapping_uv.uv_dilation_cv / remapping_uv_texture_cv, image_outpainting), CPU side: the
numpy restatement of the rule (tests/support/inpaint_ref.py) against a brute-force distance and against the properties the rule is chosen for; the measured
float32-float64 difference d that gives the GPU test its bound; the GPU test's comparison rejecting six wrong variants of the rule; signatures and refusals;
the C ABI's -2 returns before any device call.

Measured here (printed by test_bound_and_excused_share_per_case): d = max |float32 - float64| over the case list is ~4e5 uint8 steps, from ONE case, the 64 x 65
image filled from a single pixel (713 distance levels), and 4.8e-3 / 9.0e-3 on the slanted 96 x 40 hole; every other case stays below 5e-4.  The rule's
first-order extrapolation of an UNCLAMPED float working image amplifies a perturbation from level to level, so 4 d exceeds the 0.25 uint8 steps the design hoped
for by far; the per-case bound 4 d_case the tests use is never wider than 4 d."""
import inspect

import numpy as np
import pytest

from tests.support import inpaint_ref as R


def _disc_hole(n=21, r=5.5):
    y, x = np.mgrid[0:n, 0:n]
    return ((y - n // 2) ** 2 + (x - n // 2) ** 2 <= r * r).astype(np.uint8)


def test_restatement_distance_equals_brute_force():
    rng = np.random.default_rng(3)
    holes = [hole for _, _, hole, _ in R.cases()] + [_disc_hole(), (rng.uniform(0, 1, (17, 40)) < 0.9).astype(np.uint8)]
    for hole in holes:
        a, b = R.distance(hole), R.distance_brute(hole)
        assert a.dtype == np.int32 and a.tobytes() == b.tobytes(), hole.shape
    assert (R.distance(np.ones((3, 4))) == R.NONE).all() and (R.distance(np.zeros((3, 4))) == 0).all()
    # the available set is never empty: the 4-neighbour along the larger axis offset towards the nearest pixel outside the hole has a smaller D2
    d = R.distance(R.slanted_hole()).astype(np.int64)
    p = np.pad(d, 1, constant_values=R.NONE)
    nb = np.minimum(np.minimum(p[:-2, 1:-1], p[2:, 1:-1]), np.minimum(p[1:-1, :-2], p[1:-1, 2:]))
    assert (nb[d > 0] < d[d > 0]).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constant_image_fills_to_the_constant(dtype):
    for eps, C, hole in [(1, 3, _disc_hole()), (2, 1, _disc_hole(15, 4.0)), (3, 4, R.cases()[8][2]), (8, 3, R.cases()[9][2])]:
        img = np.full(hole.shape + (C,), 0, np.uint8) + np.array([7, 200, 255, 0], np.uint8)[:C]
        u, f, _ = R.telea(img, hole, eps, dtype)
        assert (u == img).all()
        assert np.abs(f.astype(np.float64) - img).max() <= 255 * 64 * np.finfo(dtype).eps      # sums of up to 196 equal terms, a few levels deep


@pytest.mark.parametrize("eps", [2, 3])
def test_affine_image_is_reproduced_to_first_order(eps):
    """I = 2 x + 3 y + 10 under a convex hole: every available pixel has an available neighbour on each axis, so its gradient is exactly (2, 3) and
    I(q) + grad I(q) . r = I(p) for every tap -- the reason for the paper's form.  What is left is the rounding of the weighted mean of (nearly) equal terms:
    at most 28 terms of size <= 133, a handful of levels deep, so 133 x 256 eps of the format bounds it generously."""
    hole = _disc_hole(21, 5.5)
    y, x = np.mgrid[0:21, 0:21]
    ref = (2 * x + 3 * y + 10).astype(np.float64)
    img = ref.astype(np.uint8)[..., None]
    for dtype in (np.float32, np.float64):
        u, f, _ = R.telea(img, hole, eps, dtype)
        err = np.abs(f[..., 0].astype(np.float64) - ref).max()
        print("affine eps %d %s: %.3g" % (eps, dtype.__name__, err))
        assert err <= 133 * 256 * np.finfo(dtype).eps
        assert (u[..., 0] == ref).all()
    # without the gradient term the fill is not first-order exact
    _, f0, _ = R.telea(img, hole, eps, np.float64, gradient=False)
    assert np.abs(f0[..., 0] - ref).max() > 1.0


def test_schedule_independence():
    for name in ("33x31 two holes closer than 2 eps, eps 3", "33x31 block across the tiles, corners, eps 8", "64x65 bands on every border",
                 "slanted 96x40 hole, eps 1", "slanted 96x40 hole, eps 3"):
        c = R.reference(name)
        u, f, sweeps = R.telea(c["img"], c["hole"], c["eps"], np.float32, schedule="sweep")
        assert u.tobytes() == c["u32"].tobytes() and f.tobytes() == c["f32"].tobytes(), name
        if name.startswith("slanted"):      # the sideways chain: more sweeps than the hole is deep (40 rows, filled from both sides: depth 20)
            print(name, "sweeps", sweeps)
            assert sweeps > 40


def test_bound_and_excused_share_per_case():
    """d per case, the bound 4 d, and the share of hole values the comparison would excuse, counted from the float64 restatement alone: under the cap of
    2 x bound + 1 % for every case"""
    worst = 0.0
    for name, img, hole, eps in R.cases():
        c = R.reference(name)
        share, cap = R.excused_share(c["f64"], hole, c["bound"]), 2 * c["bound"] + 0.01
        worst = max(worst, c["d"])
        print("%-52s d = %.3g  bound = %.3g  excused %.4f (cap %.4f)" % (name, c["d"], c["bound"], share, cap))
        assert share <= cap, name
        assert not R.compare(c["u32"], c["f32"], c["f64"], hole, c["bound"]), name      # the float32 restatement passes the GPU test's comparison
    print("d over the case list = %.3g uint8 steps, 4 d = %.3g (0.25 was hoped for)" % (worst, 4 * worst))
    stable = [R.reference(n)["d"] for n, _, _, _ in R.cases() if not n.startswith(("slanted", "64x65 everything except"))]
    assert max(stable) < 1e-3


def test_comparison_rejects_wrong_rules():
    hole = _disc_hole(21, 5.5)
    rng = np.random.default_rng(11)
    img = R._image(rng, 21, 21, 3)
    eps = 2
    _, f64, _ = R.telea(img, hole, eps, np.float64)
    u32, f32, _ = R.telea(img, hole, eps, np.float32)
    bound = 4 * float(np.abs(f32.astype(np.float64) - f64).max())
    assert bound < 1e-2 and not R.compare(u32, f32, f64, hole, bound)
    wrong = dict(le_for_lt=dict(strict=False), no_gradient=dict(gradient=False), city_block=dict(metric="cityblock"), square_window=dict(window="square"),
                 r_swapped=dict(swap_r=True))
    for name, kw in wrong.items():
        u, f, _ = R.telea(img, hole, eps, np.float32, **kw)
        bad = R.compare(u, f, f64, hole, bound)
        print(name, bad)
        assert bad, name
    # round-half-up: a single pixel between 0 and 1 is exactly 0.5 (equal weights on both sides), which rounds to 0
    img = np.array([[0, 0, 0, 0, 9, 1, 1, 1, 1]], np.uint8)[..., None]
    hole = np.zeros((1, 9), np.uint8)
    hole[0, 4] = 1
    _, f64, _ = R.telea(img, hole, 1, np.float64)
    u, f, _ = R.telea(img, hole, 1, np.float32)
    assert f[0, 4, 0] == 0.5 and u[0, 4, 0] == 0 and not [b for b in R.compare(u, f, f64, hole, 1e-6) if "half-even" in b]
    u, f, _ = R.telea(img, hole, 1, np.float32, rounding="up")
    assert u[0, 4, 0] == 1 and [b for b in R.compare(u, f, f64, hole, 1e-6) if "half-even" in b]


def test_signatures_defaults_and_refusals():
    import torch
    from unitex_amd.texturetools import image_outpainting as IO, ops, remapping_uv as RU
    sig = inspect.signature(RU.remapping_uv_texture_cv)
    assert sig == inspect.signature(RU.remapping_uv_texture)
    dflt = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert dflt == dict(map_Kd=None, weights=None, use_alpha=True, overlay_confidence=0.2, use_blending=True, blending_type="soft", blending_confidence=0.2,
                        use_inpainting=True, use_cv_inpainting=True, inpainting_confidence=0.2, use_outpainting=True, use_cv_outpainting=False, render_size=512,
                        texture_size=1024, visualize=False, perspective=True, return_stages=False)
    sig = inspect.signature(RU.uv_dilation_cv)
    assert list(sig.parameters) == ["map_Kd", "map_mask", "max_iters"] and sig.parameters["max_iters"].default == -1
    sig = inspect.signature(IO.image_outpainting)
    assert list(sig.parameters) == ["src", "mask", "n_erode_pix", "n_radius", "method"]
    assert [sig.parameters[k].default for k in ("n_erode_pix", "n_radius", "method")] == [0, 1, "ns"]
    sig = inspect.signature(ops.inpaint_telea)
    assert list(sig.parameters)[:5] == ["img_u8", "hole_u8", "radius", "return_float", "trace"]
    assert [sig.parameters[k].default for k in ("radius", "return_float", "trace")] == [1, False, None]
    src, mask = torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, 1)
    with pytest.raises(NotImplementedError, match="'telea'"):
        IO.image_outpainting(src, mask)
    with pytest.raises(ValueError, match="method"):
        IO.image_outpainting(src, mask, method="fmm")
    c2ws = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    args = (None, c2ws, np.eye(3, dtype=np.float32), np.zeros((3, 4, 8, 8), np.float32))
    # the old name keeps its three refusals ...
    with pytest.raises(NotImplementedError, match="use_cv_inpainting=False"):
        RU.remapping_uv_texture(*args)
    with pytest.raises(NotImplementedError, match="use_cv_outpainting"):
        RU.remapping_uv_texture(*args, use_cv_inpainting=False, use_cv_outpainting=True)
    with pytest.raises(NotImplementedError, match="poisson"):
        RU.remapping_uv_texture(*args, use_cv_inpainting=False, blending_type="poisson")
    # ... the new one refuses visualize only, keeps the reference's two assertions, and gets as far as the mesh with everything else
    with pytest.raises(NotImplementedError, match="visualize"):
        RU.remapping_uv_texture_cv(*args, visualize=True)
    with pytest.raises(ValueError, match="size mismatch: length of weights should be 3 but 2"):
        RU.remapping_uv_texture_cv(*args, weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="value error: linear is not supported"):
        RU.remapping_uv_texture_cv(*args, blending_type="linear")
    for kw in (dict(), dict(use_cv_outpainting=True), dict(blending_type="poisson")):
        with pytest.raises(TypeError):
            RU.remapping_uv_texture_cv(*args, **kw)      # mesh is neither a DeviceMesh nor a renderer
    from unitex_amd.texturetools import image_fusion as IF
    with pytest.raises(NotImplementedError):
        IF.smooth_fusion()
    with pytest.raises(ValueError, match="radius"):
        ops.inpaint_telea(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8), radius=9)


def test_c_abi_refuses_bad_arguments_before_any_device_call():
    import ctypes as C
    from unitex_amd import _lib
    lib = _lib.load_library()
    for name, nargs in (("utx_inpaint_distance", 7), ("utx_inpaint_telea_step", 12), ("utx_inpaint_finish", 8)):
        assert len(_lib.SYMBOLS[name][1]) == nargs
    buf = (C.c_char * 4096)()
    a = C.addressof(buf)
    p = lambda off=0: C.c_void_p(a + off)
    dist, step, fin = lib.utx_inpaint_distance, lib.utx_inpaint_telea_step, lib.utx_inpaint_finish
    assert dist(None, None, 4, 4, p(256), p(512), None) == -2 and dist(None, p(), 0, 4, p(256), p(512), None) == -2
    assert dist(None, p(), 4, 4, p(256), p(256), None) == -2 and dist(None, p(), 4, 16385, p(256), p(512), None) == -2
    good = dict(col_in=p(), done_in=p(1024), d2=p(2048), H=4, W=4, C=3, radius=1, col_out=p(256), done_out=p(1280), counter=p(3072))
    call = lambda **k: step(None, *[{**good, **k}[n] for n in ("col_in", "done_in", "d2", "H", "W", "C", "radius", "col_out", "done_out", "counter")], None)
    for k in (dict(C=0), dict(C=5), dict(radius=0), dict(radius=9), dict(radius=-1), dict(H=0), dict(W=0), dict(col_in=None), dict(done_in=None), dict(d2=None),
              dict(col_out=None), dict(done_out=None), dict(counter=None), dict(col_out=p()), dict(done_out=p(1024)), dict(counter=p(3073))):
        assert call(**k) == -2, k
    assert fin(None, None, 4, 4, 3, p(256), None, None) == -2 and fin(None, p(), 4, 4, 5, p(256), None, None) == -2
    assert fin(None, p(), 0, 4, 3, p(256), None, None) == -2 and fin(None, p(), 4, 4, 3, None, None, None) == -2 and fin(None, p(), 4, 4, 3, p(256), p(), None) == -2
