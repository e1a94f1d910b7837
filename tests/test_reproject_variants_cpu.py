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
from tests import test_perspective_cpu as PC

F32 = np.float32
PRIORITY = [0, 3, 4, 1, 2, 5]


# ---------------------------------------------------------------------------------------------------
# restatements (the HIP kernels' formulation)
# ---------------------------------------------------------------------------------------------------
def _window(a, r, op, axis):
    """op over the in-image texels of a 2r+1 window along axis (out-of-image texels skipped)"""
    out = a.copy()
    n = a.shape[axis]
    for d in range(1, r + 1):
        if d >= n:
            break
        lo = [slice(None)] * a.ndim
        hi = [slice(None)] * a.ndim
        lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
        out[tuple(lo)] = op(out[tuple(lo)], a[tuple(hi)])
        out[tuple(hi)] = op(out[tuple(hi)], a[tuple(lo)])
    return out


def window2(a, r, op):
    return _window(_window(a, r, op, 1), r, op, 0)


def seam_identity(winner, cov, k_boundary=3, k_boundary_blur=3):
    """utx_seam_mask_sized: bnd = the (2 rb + 1)^2 window's min or max winner differs from the texel's; seam = dilate_rd(bnd) AND erode_(rd+2)(cov)"""
    rb, rd = k_boundary // 2, k_boundary_blur // 2
    w = np.asarray(winner, np.int32)
    bnd = (window2(w, rb, np.minimum) != w) | (window2(w, rb, np.maximum) != w)
    return window2(bnd, rd, np.logical_or) & window2(np.asarray(cov, bool), rd + 2, np.logical_and)


def seam_reference_loop(vis, cov, k_boundary=3, k_boundary_blur=3, order=PRIORITY):
    """bake_mv_to_uv_reproject_blur's seam, restated with torch on the CPU as the reference writes it (per-view get_boundary_mask, max_pool2d)"""
    vis = torch.from_numpy(np.asarray(vis, bool))[..., None]
    mask_2d = torch.from_numpy(np.asarray(cov, bool))[None, ..., None]
    mp = torch.nn.functional.max_pool2d

    def get_boundary_mask(m, kernel_size):
        a = m.to(torch.float32)
        inner = (a - (1.0 - mp(1.0 - a.permute(0, 3, 1, 2), 2 * (kernel_size // 2) + 1, 1, kernel_size // 2)).permute(0, 2, 3, 1) > 0)
        outer = (mp(a.permute(0, 3, 1, 2), 2 * (kernel_size // 2) + 1, 1, kernel_size // 2).permute(0, 2, 3, 1) - a > 0)
        return torch.logical_or(inner, outer)
    cur = torch.zeros_like(vis[:1])
    bnd = torch.zeros_like(vis[:1])
    for i in order:
        extra = torch.logical_and(cur.logical_not(), vis[[i]])
        cur = torch.logical_or(cur, extra)
        bnd = torch.logical_or(bnd, get_boundary_mask(extra, k_boundary))
    kbb = k_boundary_blur
    bnd = mp(bnd.to(torch.float32).permute(0, 3, 1, 2), 2 * (kbb // 2) + 1, 1, kbb // 2).permute(0, 2, 3, 1) > 0
    ero = 1.0 - mp(1.0 - mask_2d.to(torch.float32).permute(0, 3, 1, 2), 2 * (kbb // 2) + 5, 1, kbb // 2 + 2).permute(0, 2, 3, 1) > 0
    return torch.logical_and(ero, bnd)[0, ..., 0].numpy()


def winner_of(vis, order=PRIORITY):
    w = np.full(vis.shape[1:], -1, np.int32)
    for v in reversed(order):
        w[vis[v]] = v
    return w


def gaussian_w1(k):
    """torchvision's _get_gaussian_kernel1d with sigma = 0.15 k + 0.35, torch float32 on the CPU"""
    sigma = k * 0.15 + 0.35
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return (pdf / pdf.sum()).numpy()


def gaussian_blur_fp64(img_hwc, k, seam=None):
    """utx_gaussian_blur_seam in fp64: weights w1[i] * w1[j] rounded to fp32 once, reflect padding of k // 2, depthwise; src where seam is 0"""
    w1 = gaussian_w1(k)
    w2 = (w1[:, None] * w1[None, :]).astype(F32).astype(np.float64)
    r = k // 2
    src = np.asarray(img_hwc, F32)
    p = np.pad(src.astype(np.float64), ((r, r), (r, r), (0, 0)), mode="reflect")
    H, W = src.shape[:2]
    out = np.zeros(src.shape, np.float64)
    for i in range(k):
        for j in range(k):
            out += w2[i, j] * p[i:i + H, j:j + W]
    if seam is None:
        return out
    return np.where(np.asarray(seam, bool)[..., None], out, src.astype(np.float64))


def torchvision_blur(img_hwc, k):
    """torchvision's tensor path: torch.mm of the 1-D weights, F.pad(mode='reflect'), depthwise conv2d (float32, CPU)"""
    w1 = torch.from_numpy(gaussian_w1(k))
    kernel = torch.mm(w1[:, None], w1[None, :]).expand(3, 1, k, k)
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(img_hwc, F32).transpose(2, 0, 1)))[None]
    x = torch.nn.functional.pad(x, [k // 2] * 4, mode="reflect")
    return torch.nn.functional.conv2d(x, kernel, groups=3)[0].numpy().transpose(1, 2, 0)


def sample_wrap(img, gx, gy):
    """nvdiffrast's linear 2-D lookup with the wrap boundary in float32, the kernel's operation order: img [H,W,C], gx/gy ndc -> [..., C]"""
    H, W = img.shape[:2]
    gx, gy = np.asarray(gx, F32), np.asarray(gy, F32)
    fin = np.isfinite(gx) & np.isfinite(gy)
    u = np.where(fin, gx, F32(0)) * F32(0.5) + F32(0.5)
    v = np.where(fin, gy, F32(0)) * F32(0.5) + F32(0.5)
    u = u - np.floor(u)
    v = v - np.floor(v)
    u = u * F32(W) - F32(0.5)
    v = v * F32(H) - F32(0.5)
    fu0, fv0 = np.floor(u), np.floor(v)
    fu, fv = (u - fu0)[..., None], (v - fv0)[..., None]
    iu0, iv0 = fu0.astype(np.int64), fv0.astype(np.int64)
    iu1, iv1 = iu0 + 1, iv0 + 1
    iu0 = np.where(iu0 < 0, iu0 + W, iu0)
    iv0 = np.where(iv0 < 0, iv0 + H, iv0)
    iu1 = np.where(iu1 >= W, iu1 - W, iu1)
    iv1 = np.where(iv1 >= H, iv1 - H, iv1)
    lerp = lambda a, b, t: (a + t * (b - a)).astype(F32)
    out = lerp(lerp(img[iv0, iu0], img[iv0, iu1], fu), lerp(img[iv1, iu0], img[iv1, iu1], fu), fv)
    return np.where(fin[..., None], out, F32(0)).astype(F32)


def backproject_nvdiff(rast2d, verts, faces, fn, vndc, images4, rayvis):
    """utx_backproject_sampled(sample_mode=1) without the rays: colour [n,Th,Tw,3], alphaok [n,Th,Tw] u8 (rayvis comes from the ray model)"""
    n = images4.shape[0]
    cov = rast2d[..., 3] > 0
    col = np.zeros((n,) + cov.shape + (3,), F32)
    ao = np.zeros((n,) + cov.shape, np.uint8)
    for v in range(n):
        g = G.interpolate(np.ascontiguousarray(vndc[v], F32), rast2d, faces)[cov]      # (a0 u + a1 v) + a2 w, the kernel's order
        s = sample_wrap(images4[v], g[:, 0], g[:, 1])
        col[v][cov] = s[:, :3]
        ao[v][cov] = (s[:, 3] > F32(0.999)).astype(np.uint8)
    return col, ao


def scene(f, tag):
    """the G67n scene of set tag ('o' orthographic, 'p' perspective)"""
    persp = tag == "p"
    verts, faces, uvs, c2ws, intr = f["verts"], f["faces"], f["uvs"], f["c2ws_" + tag], f["intr_" + tag]
    clip = G.transform_points(verts, G.mvp_matrices(c2ws, intr, perspective=persp))
    uvclip = np.concatenate([uvs * 2 - 1, np.zeros((len(uvs), 1), F32), np.ones((len(uvs), 1), F32)], -1)
    return dict(verts=verts, faces=faces, clip=clip, vndc=(clip[..., :2] / clip[..., 3:4]).astype(F32), uvclip=uvclip, persp=persp,
                fn=G.face_normals(verts, faces), eyes=np.ascontiguousarray(c2ws[:, :3, 3], F32), dirs=(-c2ws[:, :3, 2]).astype(F32))


def texel_layers(s, T, images4, angle_deg, sample):
    """(rast2d, rayvis, alphaok, colour, dilated visibility) of uv_to_pcd; sample 'grid' (the oracle's gather) or 'nvdiff' (sample_wrap)"""
    rast2d = G.rasterize(s["uvclip"], s["faces"], T, T)
    bvh = G.BVH(s["verts"], s["faces"])
    col, rv, ao = G.backproject(rast2d, s["verts"], s["faces"], s["fn"], s["vndc"], s["dirs"], images4, bvh, angle_deg=angle_deg)
    if s["persp"]:
        rv = PC.texel_rayvis(rast2d, s["verts"], s["faces"], s["fn"], s["eyes"], bvh, angle_deg)
    if sample == "nvdiff":
        col, ao = backproject_nvdiff(rast2d, s["verts"], s["faces"], s["fn"], s["vndc"], images4, rv)
    return rast2d, rv, ao, col, G.dilate_visibility(rv, rast2d[..., 3] > 0, ao)


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
