"""Back-projection variants, CPU side: numpy restatements of the three new pieces -- the seam mask at any window sizes, the Gaussian seam blur
(torchvision's gaussian_blur, reflect padding) and nvdiffrast's linear texture lookup with the wrap boundary -- checked against the reference's
formulation and against its own outputs (fixtures G67g / G67n, tests/golden/make_golden_reproject_variants.py).

Reference (TextureTools/texturetools/render/nvdiffrast/renderer_inverse.py): bake_mv_to_uv_reproject_blur ORs, over the views in priority order,
get_boundary_mask(newly claimed region, kernel_size_boundary) (:596-602, :435-444), dilates it by max_pool2d(2 (kbb // 2) + 1) and ANDs the coverage
eroded by 2 (kbb // 2) + 5 (:603-604); method='gaussian' blurs with gaussian_blur(img, (k, k)) (:618-619); uv_to_pcd(grid_interpolate_mode='nvdiff')
samples the views with dr.texture(ndc * 0.5 + 0.5, filter_mode='linear') (:299-305)."""
import numpy as np
import pytest
import torch

from oracle import geom_ref as G
from oracle import reproject_ref as PC
from oracle.pixel_ref import sample_wrap
from oracle.reproject_ref import gaussian_blur_fp64, gaussian_w1, scene, seam_identity, seam_reference_loop, texel_layers, torchvision_blur, winner_of

F32 = np.float32


# ---------------------------------------------------------------------------------------------------
SIZES = [(3, 3), (5, 5), (1, 3), (3, 1), (0, 0), (7, 4), (2, 9), (31, 31), (30, 17)]


def test_seam_identity_equals_the_reference_loop_on_g67g():
    f = PC.load("g67g_reproject_gaussian.npz")
    n, T = 6, 96
    vis = PC.unpack(f["mask_2d_visiable"], (n, T, T, 1))[..., 0]
    cov = PC.unpack(f["mask_2d"], (1, T, T, 1))[0, ..., 0]
    w = winner_of(vis)
    seams = {}
    for kb, kbb in SIZES:
        ref = seam_reference_loop(vis, cov, kb, kbb)
        assert np.array_equal(seam_identity(w, cov, kb, kbb), ref), "seam at (%d, %d)" % (kb, kbb)
        seams[(kb, kbb)] = ref
    assert seams[(3, 3)].sum() > 200 and not np.array_equal(seams[(3, 3)], seams[(5, 5)])
    # the oracle's 3 / 3 formulation (per-view boundary union, 3x3 dilation, 7x7 erosion) is the same mask
    _, _, _, bnd = G.composite(np.zeros((n, T, T, 3), F32), vis)
    assert np.array_equal(seams[(3, 3)], G.seam_mask(bnd, cov))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seam_identity_equals_the_reference_loop_on_random_winner_maps(seed):
    """37 x 53 maps of blobs (so boundaries are sparse) with seams on the image edge, coverage with holes and covered edges"""
    rng = np.random.default_rng(seed)
    H, W = 37, 53
    yy, xx = np.mgrid[0:H, 0:W]
    w = np.full((H, W), -1, np.int32)
    for _ in range(14):
        cy, cx, r = rng.integers(-3, H + 3), rng.integers(-3, W + 3), rng.integers(2, 12)
        w[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = rng.integers(-1, 6)
    cov = np.ones((H, W), bool)
    for _ in range(4):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, 5)
        cov[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = False
    w[~cov] = -1
    vis = np.stack([w == v for v in range(6)])
    assert (w[0] != w[0, 0]).any() or (w[:, 0] != w[0, 0]).any(), "a seam must reach the image edge"
    for kb, kbb in SIZES + [(rng.integers(0, 32), rng.integers(0, 32)) for _ in range(3)]:
        assert np.array_equal(seam_identity(w, cov, kb, kbb), seam_reference_loop(vis, cov, kb, kbb)), "seam at (%d, %d)" % (kb, kbb)


@pytest.mark.parametrize("k", [1, 3, 5, 7, 9, 15, 31])
def test_gaussian_weights_equal_torch_bit_for_bit(k):
    from unitex_amd.texturetools import ops
    w1 = ops.gaussian_kernel1d(k).numpy()
    assert w1.dtype == F32 and np.array_equal(w1, gaussian_w1(k))
    t = torch.from_numpy(w1)
    # the kernel's 2-D weight is the one fp32 product w1[i] * w1[j]: the same bits as torchvision's torch.mm of [k, 1] x [1, k]
    assert np.array_equal(torch.mm(t[:, None], t[None, :]).numpy(), (w1[:, None] * w1[None, :]).astype(F32))
    assert abs(float(w1.astype(np.float64).sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("k", [1, 3, 5, 7, 31])
def test_gaussian_blur_restatement_matches_torchvision_form(k):
    rng = np.random.default_rng(k)
    img = rng.random((40, 35, 3)).astype(F32)
    ref = torchvision_blur(img, k)
    got = gaussian_blur_fp64(img, k)
    assert np.abs(got - ref).max() < 4e-6      # torch's fp32 conv sums k^2 taps in fp32 (1.1e-6 from the fp64 sum at k = 31)
    if k > 1:
        # reflect, not symmetric: the edge texel is not repeated, which shows on the border rows
        r = k // 2
        sym = np.pad(img.astype(np.float64), ((r, r), (r, r), (0, 0)), mode="symmetric")
        w2 = np.outer(gaussian_w1(k), gaussian_w1(k)).astype(F32).astype(np.float64)
        sym_row0 = sum(w2[i, j] * sym[i, j:j + 35] for i in range(k) for j in range(k))
        assert np.abs(sym_row0 - ref[0]).max() > 1e-4


def test_wrap_sampling_restatement():
    """sample_wrap on hand-checked coordinates: the border half-texel takes the opposite edge, u = 1 wraps to 0, non-finite samples zero"""
    img = np.arange(4 * 5 * 1, dtype=F32).reshape(4, 5, 1)
    # the texel centre of (x=2, y=1): u = (2 + 0.5) / 5, gx = 2u - 1
    gx, gy = F32(2 * 2.5 / 5 - 1), F32(2 * 1.5 / 4 - 1)
    assert sample_wrap(img, gx, gy)[..., 0] == img[1, 2, 0]
    # left border (gx = -1): halfway between column 4 (wrapped) and column 0
    got = sample_wrap(img, F32(-1), F32(2 * 1.5 / 4 - 1))[..., 0]
    assert got == F32(0.5) * (img[1, 4, 0] + img[1, 0, 0])
    assert sample_wrap(img, F32(1), F32(2 * 1.5 / 4 - 1))[..., 0] == got
    assert (sample_wrap(img, np.array([np.nan, np.inf], F32), np.array([0, 0], F32)) == 0).all()


@pytest.mark.parametrize("tag", ["o", "p"])
def test_g67n_nvdiff_texel_visibility_matches_reference(tag):
    f = PC.load("g67n_backprojection_nvdiff.npz")
    s = scene(f, tag)
    imgs = f["images"].astype(F32)
    n, HW = imgs.shape[:2]
    T = 96
    mv_alpha = np.stack([G.rasterize(s["clip"][v], s["faces"], HW, HW)[..., 3] > 0 for v in range(n)])
    assert np.array_equal(mv_alpha, PC.unpack(f["mv_alpha_" + tag], (n, HW, HW, 1))[..., 0]), "view coverage"
    alpha = PC.unpack(f["alpha_" + tag], (n, HW, HW, 1)).astype(F32)
    images4 = np.concatenate([imgs, alpha], -1)
    rast2d, rv, ao, col, vis = texel_layers(s, T, images4, 100.0, "nvdiff")
    assert np.array_equal(rast2d[..., 3] > 0, PC.unpack(f["mask_2d_" + tag], (1, T, T, 1))[0, ..., 0])
    ref = PC.unpack(f["mask_2d_visiable_" + tag], (n, T, T, 1))[..., 0]
    mism = int((vis != ref).sum())
    print("G67n %s texel visibility (nvdiff): %d of %d differ" % (tag, mism, ref.size))
    assert mism <= 4
    # the sampling matters: grid_sample's zero padding sees another set of texels, as the reference's own 'torch' run does
    _, _, _, _, vis_t = texel_layers(s, T, images4, 100.0, "grid")
    ref_t = PC.unpack(f["mask_2d_visiable_torch_" + tag], (n, T, T, 1))[..., 0]
    assert int((vis_t != ref_t).sum()) <= 4
    assert int((vis_t != vis).sum()) >= 20
    if tag == "p":
        both = vis & ref
        ref_cols = np.zeros((n, T, T, 3), F32)
        ref_cols[ref] = f["vis_colors_p"]
        assert np.abs(ref_cols[both] - col[both]).max() < 2e-6, "wrap-sampled colours"
