"""Back-projection variants (TEST INFRASTRUCTURE ONLY): the numpy restatements, in the HIP kernels' operation order, that geom_ref.py's default path
does not cover -- the reference's perspective ray model (utx_backproject_persp, utx_view_visibility_persp), the seam mask at any window sizes, the
Gaussian seam blur (torchvision's gaussian_blur, reflect padding), nvdiffrast's linear texture lookup with the wrap boundary (oracle/pixel_ref.py),
and what the nine-channel (PBR stack) bake shares between its CPU and GPU tests.  Pinned against the reference's own outputs by
tests/test_perspective_cpu.py (fixtures G67p / G11p / G9p, tests/golden/make_golden_perspective.py), tests/test_reproject_variants_cpu.py (G67g /
G67n, tests/golden/make_golden_reproject_variants.py) and tests/test_pbr_stack_cpu.py (G67s, tests/golden/make_golden_pbr_stack.py).

Reference (TextureTools/texturetools/render/nvdiffrast/renderer_inverse.py): with perspective=True every ray of a view starts at the camera
centre c2w[:3, 3] and points at the surface point, rays_d = normalize(pos - rays_o) = x / max(|x|, 1e-12) (:187-190 view pixels, :279-285 texels);
a texel is seen when the closest hit is its own face and cosine_similarity(rays_d, face normal) < cos(threshold).  bake_mv_to_uv_reproject_blur ORs,
over the views in priority order, get_boundary_mask(newly claimed region, kernel_size_boundary) (:596-602, :435-444), dilates it by
max_pool2d(2 (kbb // 2) + 1) and ANDs the coverage eroded by 2 (kbb // 2) + 5 (:603-604); method='gaussian' blurs with gaussian_blur(img, (k, k))
(:618-619); uv_to_pcd(grid_interpolate_mode='nvdiff') samples the views with dr.texture(ndc * 0.5 + 0.5, filter_mode='linear') (:299-305)."""
import math
import os

import numpy as np
import torch

from . import geom_ref as G
from .geom_ref import PRIORITY
from .pixel_ref import sample_wrap

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
F32 = np.float32


def load(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def unpack(a, shape):
    return np.unpackbits(a)[:int(np.prod(shape))].reshape(shape).astype(bool)


def persp_dirs(pos, eye):
    """pos [..., 3], eye [3] -> (pos - eye) / max(sqrt((x*x + y*y) + z*z), 1e-12), float32, the kernels' order"""
    pos, eye = np.asarray(pos, F32), np.asarray(eye, F32)
    x, y, z = pos[..., 0] - eye[0], pos[..., 1] - eye[1], pos[..., 2] - eye[2]
    n = np.maximum(np.sqrt((x * x + y * y) + z * z), F32(1e-12))
    return np.stack([x / n, y / n, z / n], -1).astype(F32)


def facing(d, fn, angle_deg):
    """cosine_similarity(d, fn) < cos(angle) with eps 1e-8 on both norms: the shared cosine expression of the kernels"""
    d, fn = np.asarray(d, F32), np.asarray(fn, F32)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    ld = np.maximum(np.sqrt(dot(d, d)), F32(1e-8))
    ln = np.maximum(np.sqrt(dot(fn, fn)), F32(1e-8))
    return (dot(d, fn) / (ld * ln)) < F32(math.cos(math.radians(angle_deg)))


def texel_rayvis(rast2d, verts, faces, fn, eyes, bvh, angle_deg):
    """uv_to_pcd's per-texel ray test with perspective rays -> rayvis [n, Th, Tw] u8 (before the hole filling)"""
    cov = rast2d[..., 3] > 0
    tid = rast2d[..., 3].astype(np.int64)[cov] - 1
    pos = G.interpolate(verts, rast2d, faces)[cov]
    out = np.zeros((len(eyes),) + cov.shape, np.uint8)
    for v, eye in enumerate(np.asarray(eyes, F32)):
        d = persp_dirs(pos, eye)
        hit = bvh.trace(np.broadcast_to(eye, d.shape), d)
        out[v][cov] = ((hit == tid) & (hit != -1) & facing(d, fn[tid], angle_deg)).astype(np.uint8)
    return out


def view_visibility_persp(attr6, rast, fn, eyes, grad_thr=0.20, angle_deg=115.0):
    """mv_to_pcd(filt_gradient_points=True) with perspective rays: coverage AND the eroded gradient test (the oracle's view_visibility, its
    facing term switched off by zero face normals -- cosine 0 -- and an 80 degree threshold) AND the perspective facing test"""
    smooth_cov = G.view_visibility(attr6, rast, np.zeros_like(fn), np.ones((len(eyes), 3), F32), grad_thr=grad_thr, angle_deg=80.0)
    tid = np.maximum(rast[..., 3].astype(np.int64) - 1, 0)
    face = np.stack([facing(persp_dirs(attr6[v, ..., :3], e), fn[tid[v]], angle_deg) for v, e in enumerate(np.asarray(eyes, F32))])
    return smooth_cov & face


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


def scene(f, tag=None):
    """the scene of a back-projection fixture: one perspective camera set (G67p, G11p), or set `tag` of G67n ('o' orthographic, 'p' perspective)"""
    persp = tag != "o"
    verts, faces, uvs = f["verts"], f["faces"], f["uvs"]
    c2ws, intr = (f["c2ws"], f["intr"]) if tag is None else (f["c2ws_" + tag], f["intr_" + tag])
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
        rv = texel_rayvis(rast2d, s["verts"], s["faces"], s["fn"], s["eyes"], bvh, angle_deg)
    if sample == "nvdiff":
        col, ao = backproject_nvdiff(rast2d, s["verts"], s["faces"], s["fn"], s["vndc"], images4, rv)
    return rast2d, rv, ao, col, G.dilate_visibility(rv, rast2d[..., 3] > 0, ao)


def atlas_visibility(s, T, images4, angle_deg):
    """texel_layers with the oracle's gather: colour and alpha do not depend on the rays"""
    return texel_layers(s, T, images4, angle_deg, "grid")


# ---- the nine-channel (PBR stack) bake, fixture G67s
N, HW, T = 6, 48, 96


def check_atlas(name, got, ref):
    """the bounds of test_reproject_variants_gpu._check_atlas"""
    err = np.abs(got - ref)
    print("%s final atlas: max |d| %.3g, median %.3g, share beyond 1e-4: %.5f" % (name, err.max(), np.median(err), (err > 1e-4).mean()))
    assert (err > 1e-4).mean() < 2e-3 and np.median(err) < 1e-6, name


def g67s():
    f = load("g67s_pbr_stack.npz")
    imgs = f["images"].astype(F32)
    assert imgs.shape == (N, HW, HW, 9)
    alpha = unpack(f["alpha"], (N, HW, HW, 1)).astype(F32)
    return f, imgs, alpha


def _blob_winner(H, W, seed, n_blobs):
    """blobs of view ids 0..5 and -1 (texels no view sees), and coverage with holes; seams reach the image edge"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    w = torch.full((H, W), -1, dtype=torch.int8)
    for _ in range(n_blobs):
        cy, cx = int(torch.randint(-H // 10, H + H // 10, (1,), generator=g)), int(torch.randint(-W // 10, W + W // 10, (1,), generator=g))
        r = int(torch.randint(2, max(3, min(H, W) // 6), (1,), generator=g))
        w[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = int(torch.randint(-1, 6, (1,), generator=g))
    cov = torch.ones(H, W, dtype=torch.bool)
    for _ in range(n_blobs // 4):
        cy, cx = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
        r = int(torch.randint(1, max(2, min(H, W) // 20), (1,), generator=g))
        cov[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = False
    w[~cov] = -1
    rast = torch.zeros(H, W, 4)
    rast[..., 3] = cov.float()
    return w, rast
