"""Restatement (TEST INFRASTRUCTURE ONLY), written for this project, of the three stages of the vertex-colour bake (utx_view_weight_maps, utx_vertex_project with its epilogue,
utx_vertex_inpaint_step; the reference: texture/reprojection/mesh_remapping.py:508-627, :326-343) in numpy, shared by tests/test_vertex_bake_cpu.py and
tests/test_vertex_bake_gpu.py.  Every function takes dtype: np.float32 evaluates the kernels' expressions in their order, np.float64 is the yardstick the
counted bounds are measured from.  Also the bounds themselves (project_bound, ARCCOS_BOUND, inpaint_bound): roundings counted, times 2^-24 of the operand
scale, never fitted to a result."""
import math
import os

import numpy as np
import torch

from .pixel_ref import bake_epilogue, sample_planar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -24                                   # unit roundoff of float32
HALF_PI32 = np.float32(math.pi / 2)
GRAD_THR32 = np.float32(math.radians(10) / (math.pi / 2))
# device acosf on [-1, 0] against float64: the measured maximum, in ulps of the result (2^-22 on [2, pi], 2^-23 below), rounded up to a whole ulp
# (tests/test_vertex_bake_gpu.py::test_device_acosf_stays_within_the_recorded_ulps re-measures it); + 1 ulp for the reference's acos
ACOS_ULPS = 2
# |a_gpu - a_ref| for a = ((acos(c) - h) / h).clamp(0, 1): acos differs by at most (ACOS_ULPS + 1) ulps of 2^-22, the subtraction of h is exact
# (Sterbenz: h <= acos <= 2 h), the division rounds once on each side (half an ulp of a value below 1, 2^-25, taken as 2^-24 for the values at 1)
ARCCOS_BOUND = (ACOS_ULPS + 1) * 2.0 ** -22 / (math.pi / 2) + 2 * U
GRAD_EDGE = 1e-5                                 # a pixel whose float64 gradient magnitude is this close to the threshold may fall on either side


def _arccos01(c, dt):
    h = dt(HALF_PI32)
    return np.clip((np.arccos(np.clip(c, dt(-1), dt(0))) - h) / h, dt(0), dt(1)).astype(dt)


def _gradient(a, axis):
    """torch.gradient's stencil with unit spacing: central difference over 2 inside, one-sided at the borders"""
    a = np.moveaxis(a, axis, 0)
    g = np.empty_like(a)
    g[1:-1] = (a[2:] - a[:-2]) / a.dtype.type(2)
    g[0], g[-1] = a[1] - a[0], a[-1] - a[-2]
    return np.moveaxis(g, 0, axis)


def dilate(alpha, r):
    """(2 r + 1)^2 maximum with zeros outside: alpha [B,H,W]"""
    B, H, W = alpha.shape
    p = np.zeros((B, H + 2 * r, W + 2 * r), alpha.dtype)
    p[:, r:r + H, r:r + W] = alpha
    out = np.zeros_like(alpha)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = np.maximum(out, p[:, dy:dy + H, dx:dx + W])
    return out


def weight_maps(cosn, cam_nz=None, r=0, dtype=np.float32):
    """cosn [B,H,W], cam_nz [B,H,W] | None -> dict(out [B,H,W,2], arccos, grad, alpha (undilated))"""
    dt = dtype
    c = cosn.astype(dt)
    a = _arccos01(c, dt)
    dy, dx = _gradient(a, 1), _gradient(a, 2)
    grad = np.sqrt(dy * dy + dx * dx)
    alpha = (grad > dt(GRAD_THR32)).astype(dt)
    c0 = np.clip(c, dt(-1), dt(0)) if cam_nz is None else np.clip(cam_nz.astype(dt), dt(0), dt(1))
    return dict(out=np.stack([c0, dilate(alpha, r)], -1), arccos=a, grad=grad, alpha=alpha)


def _rows(m, p, dt):
    """m [4,4] applied to the rows of p [N,4]: ((m0 x + m1 y) + m2 z) + m3 w per output component"""
    m = m.astype(dt)
    return np.stack([((m[j, 0] * p[:, 0] + m[j, 1] * p[:, 1]) + m[j, 2] * p[:, 2]) + m[j, 3] * p[:, 3] for j in range(4)], -1)


def ndc(v_pos, xform, proj, dtype=np.float32):
    p = np.concatenate([v_pos.astype(dtype), np.ones((v_pos.shape[0], 1), dtype)], -1)
    clip = _rows(proj, _rows(xform, p, dtype), dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        return clip[:, :2] / clip[:, 3:4]


def vertex_project(v_pos, visible, xform, proj, images, wmap, v_rgb, weights, use_alpha=True, dtype=np.float32, detail=None):
    """-> (v_rgb_acc [V,3], v_weight_acc [V,1]); detail (a list) receives per view (counted mask, ndc)"""
    dt = dtype
    V, B = v_pos.shape[0], visible.shape[0]
    rgb0 = v_rgb.astype(dt)
    acc, wacc = np.zeros((V, 3), dt), np.zeros((V, 1), dt)
    for b in range(B):
        g = ndc(v_pos, xform[b], proj[b], dt)
        with np.errstate(invalid="ignore"):
            inside = (g[:, 0] > -1) & (g[:, 0] < 1) & (g[:, 1] > -1) & (g[:, 1] < 1)
        vis = visible[b].astype(bool)
        on = vis & inside
        gx, gy = np.where(on, g[:, 0], 0).astype(dt), np.where(on, g[:, 1], 0).astype(dt)
        s = sample_planar(images[b], gx, gy, "reflection", dt)
        q = sample_planar(np.moveaxis(wmap[b], -1, 0), gx, gy, "zeros", dt)
        a = s[3] if use_alpha else np.ones_like(s[3])
        c = (s[:3] * a[None] + rgb0.T * (dt(1) - a)[None]).T
        cs2 = q[0] * q[0]
        w = (dt(weights[b]) * (cs2 * cs2)) * (dt(1) - q[1])
        c = np.where(on[:, None], c, rgb0)
        w = np.where(on, w, dt(0))
        acc = np.where(vis[:, None], acc + w[:, None] * c, acc)
        wacc = np.where(vis[:, None], wacc + w[:, None], wacc)
        if detail is not None:
            detail.append((on, g))
    return acc, wacc


def epilogue(acc, wacc, v_rgb, overlay_confidence, blending, blending_confidence, inpainting_confidence, dtype=np.float32):
    """remapping_vertex_color :326-343 -> (overlay, blended, inpaint mask uint8 [V]); blending None | 'soft' | 'hard'.  The thresholds are float32 values in
    either dtype: a float32 tensor is compared with a Python number in float32"""
    over, out = bake_epilogue(acc, wacc, v_rgb, overlay_confidence, blending, blending_confidence, dtype)
    return over, out, (np.asarray(wacc, dtype)[:, 0] <= dtype(np.float32(inpainting_confidence))).astype(np.uint8)


def project_bound(v_pos, visible, xform, proj, images, wmap, v_rgb, weights):
    """|float32 evaluation - exact| of (v_rgb_acc, v_weight_acc), per vertex, to first order, for ANY summation order of the two 4-term dot products (the
    reference's run through a BLAS): counted per view, in float64.
      ndc     h = T p and clip = P h: a 4-term dot product is off by at most 4 U sum|terms| (3 sums + 1 product per term, gamma_4); the division adds U |ndc|
      pixel   ix = ((g + 1) size - 1) / 2: d ix = size / 2 d g + 3 U size (two roundings at scale size, the reflection's + 0.5 - 0.5 one more)
      sample  bilinear interpolation moves by at most (d ix + d iy) D, D the largest step between neighbouring texels (the reflected / zero-padded image
              included), plus 9 U max|texel| for its own arithmetic (4 weights of 3 roundings ... 4 products, 3 sums: 9 roundings on the critical path)
      colour  c = s a + v (1 - a): d c <= d s + (|s| + |v|) d a + 3 U max;  weight  w = k cos^4 (1 - al): d w <= k (4 |cos|^3 d cos + d al + 6 U)
      sums    acc += w c, wacc += w: d(w c) + 2 U |w c| per view, U |partial sum| per addition
    The bound for the difference of two such evaluations (GPU against the float32 restatement, or against the reference) is twice this."""
    V, B = v_pos.shape[0], visible.shape[0]
    p = np.concatenate([v_pos.astype(np.float64), np.ones((V, 1))], -1)
    img, wm = images.astype(np.float64), wmap.astype(np.float64)
    e_acc, e_w = np.zeros(V), np.zeros(V)
    s_acc, s_w = np.zeros(V), np.zeros(V)
    vmax = np.abs(v_rgb).max(initial=0.0)
    for b in range(B):
        T, P = np.abs(xform[b].astype(np.float64)), np.abs(proj[b].astype(np.float64))
        h = p @ xform[b].astype(np.float64).T
        eh = 4 * U * (np.abs(p) @ T.T)
        clip = h @ proj[b].astype(np.float64).T
        ec = 4 * U * (np.abs(h) @ P.T) + eh @ P.T
        with np.errstate(divide="ignore", invalid="ignore"):
            g = clip[:, :2] / clip[:, 3:4]
            eg = (ec[:, :2] + np.abs(g) * ec[:, 3:4]) / np.abs(clip[:, 3:4]) + U * np.abs(g)
        eg = np.nan_to_num(eg, nan=0.0, posinf=0.0)

        def lip(m):          # m [C,H,W]: largest step between neighbours, with the zero frame
            z = np.pad(m, ((0, 0), (1, 1), (1, 1)))
            return max(np.abs(np.diff(z, axis=1)).max(), np.abs(np.diff(z, axis=2)).max())
        Hi, Wi = img.shape[2:]
        H, W = wm.shape[1:3]
        d_img = (Wi / 2 * eg[:, 0] + Hi / 2 * eg[:, 1] + 3 * U * (Wi + Hi)) * lip(img[b]) + 9 * U * np.abs(img[b]).max()
        d_wm = (W / 2 * eg[:, 0] + H / 2 * eg[:, 1] + 3 * U * (W + H)) * lip(np.moveaxis(wm[b], -1, 0)) + 9 * U * np.abs(wm[b]).max()
        smax = np.abs(img[b, :3]).max()
        dc = d_img + (smax + vmax) * d_img + 3 * U * max(smax, vmax)
        k = abs(float(weights[b]))
        cmax = np.abs(wm[b, ..., 0]).max()
        wmaxv = k * cmax ** 4
        dw = k * (4 * cmax ** 3 * d_wm + d_wm + 6 * U)
        on = visible[b].astype(bool)
        cm = max(smax, vmax)
        s_acc = s_acc + on * wmaxv * cm
        s_w = s_w + on * wmaxv
        e_acc = e_acc + on * (dw * cm + wmaxv * dc + 2 * U * wmaxv * cm + U * s_acc)
        e_w = e_w + on * (dw + U * s_w)
    return e_acc, e_w


def adjacency_dense(faces, V):
    A = np.zeros((V, V), bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        A[faces[:, a], faces[:, b]] = True
        A[faces[:, b], faces[:, a]] = True
    A[np.arange(V), np.arange(V)] = False
    return A


def csr_from_dense(A):
    rowptr = np.concatenate([[0], np.cumsum(A.sum(1))]).astype(np.int32)
    col = np.nonzero(A)[1].astype(np.int32)
    return rowptr, col


def inpaint(rowptr, col, v_rgb, idx, max_iters=1000, dtype=np.float32):
    """inpainting_vertex_color on a CSR adjacency -> (v_rgb, steps, [mask after each step])"""
    dt = dtype
    rgb = v_rgb.astype(dt).copy()
    V = rgb.shape[0]
    mask = np.ones(V, bool)
    mask[idx] = False
    count, steps, masks = 0, 0, []
    if len(idx) == 0:
        return rgb, 0, masks
    for _ in range(max_iters):
        new_rgb, new_mask = rgb.copy(), mask.copy()
        for v in idx:
            nb = col[rowptr[v]:rowptr[v + 1]]
            deg = dt(len(nb))
            s, m = np.zeros(3, dt), dt(0)
            for j in nb:
                if mask[j]:
                    s = s + rgb[j]
                    m = m + dt(1)
            den = deg * m
            if den > 0:
                new_rgb[v] = (deg * s) / den
            new_mask[v] = den > 0
        rgb, mask = new_rgb, new_mask
        steps += 1
        masks.append(mask.copy())
        now = int(mask[idx].sum())
        if now <= count:
            break
        count = now
    return rgb, steps, masks


def bfs_depth(rowptr, col, seeds_mask):
    """distance of every vertex from the valid set along the graph (-1: unreachable)"""
    V = len(rowptr) - 1
    dist = np.where(seeds_mask, 0, -1)
    frontier = list(np.nonzero(seeds_mask)[0])
    d = 0
    while frontier:
        d += 1
        nxt = []
        for v in frontier:
            for j in col[rowptr[v]:rowptr[v + 1]]:
                if dist[j] < 0:
                    dist[j] = d
                    nxt.append(j)
        frontier = nxt
    return dist


def inpaint_bound(steps, d_max):
    """colours in [0, 1]: a step is an average (it amplifies no earlier error) of at most d_max terms in an order torch's sparse product does not fix:
    d_max - 1 sums, the product with deg, the product deg * M (exact: small integers), the division -> at most d_max + 3 roundings of 2^-24 per step"""
    return steps * (d_max + 3) * U


def synthetic_case(V, B, seed, Hi=5, Wi=7, H=6, W=9, dead_vertex=None, dead_view=None):
    """a projection problem without a mesh: vertices scattered over and a little beyond the views, per-view similarity transforms, a perspective-like and an
    orthographic-like projection in turn, random rgba with alpha 0, 1 and between, a weight map with cos in [-1, 0] and a 0 / 1 edge alpha.
    dead_vertex: visible nowhere; dead_view: sees nothing."""
    rng = np.random.default_rng(seed)
    v_pos = rng.uniform(-1.1, 1.1, (V, 3)).astype(np.float32)
    xform = np.zeros((B, 4, 4), np.float32)
    proj = np.zeros((B, 4, 4), np.float32)
    for b in range(B):
        t = rng.uniform(-0.4, 0.4)
        xform[b] = np.array([[math.cos(t), -math.sin(t), 0, rng.uniform(-0.1, 0.1)], [math.sin(t), math.cos(t), 0, rng.uniform(-0.1, 0.1)],
                             [0, 0, 1, -3.0], [0, 0, 0, 1]], np.float32)
        if b % 2 == 0:      # perspective-like: w = -z
            proj[b] = np.array([[2.6, 0, 0.05, 0], [0, -2.6, 0.02, 0], [0, 0, -1.0, -0.02], [0, 0, -1, 0]], np.float32)
        else:
            proj[b] = np.array([[0.9, 0, 0, 0.03], [0, -0.9, 0, -0.02], [0, 0, -0.002, -1.0], [0, 0, 0, 1]], np.float32)
    images = rng.uniform(0, 1, (B, 4, Hi, Wi)).astype(np.float32)
    sel = rng.uniform(0, 1, (B, Hi, Wi))
    images[:, 3] = np.where(sel < 0.3, 0.0, np.where(sel < 0.6, 1.0, images[:, 3]))
    wmap = np.stack([rng.uniform(-1, 0, (B, H, W)), (rng.uniform(0, 1, (B, H, W)) < 0.25).astype(np.float64)], -1).astype(np.float32)
    visible = (rng.uniform(0, 1, (B, V)) < 0.7).astype(np.uint8)
    if dead_vertex is not None:
        visible[:, dead_vertex] = 0
    if dead_view is not None:
        visible[dead_view] = 0
    v_rgb = rng.uniform(0, 1, (V, 3)).astype(np.float32)
    weights = rng.uniform(0.05, 2.0, B).astype(np.float32)
    return dict(v_pos=v_pos, visible=visible, xform=xform, proj=proj, images=images, wmap=wmap, v_rgb=v_rgb, weights=weights)


# ---- torch compositions and test inputs shared by the CPU and GPU modules
def _cos_image(B, H, W, seed):
    """a cos_ray_normal-like image: smooth facing term with a few creases and a background of 0, so that both alpha classes occur"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    out = np.zeros((B, H, W), np.float32)
    for b in range(B):
        r2 = (x - rng.uniform(-0.2, 0.2)) ** 2 + (y - rng.uniform(-0.2, 0.2)) ** 2
        c = -np.sqrt(np.clip(1 - r2 / 0.8, 0, 1))
        c = np.where(x * rng.uniform(-1, 1) + y > 0.3, c * 0.5, c)
        out[b] = c.astype(np.float32)
    return out


def _torch_weight_maps(cosn, cam_nz, r):
    """mesh_remapping.py:544-555 with torch's CPU operators"""
    c = torch.from_numpy(cosn)[..., None]
    images_cos = c.clamp(-1.0, 0.0)
    arccos = ((torch.arccos(images_cos) - torch.pi / 2) / (torch.pi / 2)).clamp(0.0, 1.0)
    dy, dx = torch.gradient(arccos, dim=[1, 2])
    grad = torch.sqrt(dy.square() + dx.square())
    alpha = (grad > math.radians(10) / (math.pi / 2)).float()
    k = 2 * r + 1
    if k > 1:
        alpha = torch.nn.functional.max_pool2d(alpha.permute(0, 3, 1, 2), k, 1, k // 2).permute(0, 2, 3, 1)
    if cam_nz is not None:
        images_cos = torch.from_numpy(cam_nz)[..., None].clamp(0.0, 1.0)
    return torch.cat([images_cos, alpha], -1).numpy(), arccos[..., 0].numpy()


def _hand_points(Hi, Wi):
    """NDC points: exact pixel centres, exact halves between them, +-(1 - 2^-20), the outer half-pixel rim on all four sides"""
    e = 1 - 2.0 ** -20
    xs = [(2 * i + 1) / Wi - 1 for i in range(Wi)] + [2 * i / Wi - 1 for i in range(1, Wi)] + [-e, e, -1 + 0.5 / Wi, 1 - 0.5 / Wi, -1 + 0.25 / Wi, 1 - 0.75 / Wi, 0.0]
    ys = [(2 * i + 1) / Hi - 1 for i in range(Hi)] + [2 * i / Hi - 1 for i in range(1, Hi)] + [-e, e, -1 + 0.5 / Hi, 1 - 0.5 / Hi, -1 + 0.25 / Hi, 1 - 0.75 / Hi, 0.0]
    gx, gy = np.meshgrid(np.array(xs, np.float32), np.array(ys, np.float32))
    return gx.reshape(-1), gy.reshape(-1)


def _torch_project(case, use_alpha):
    """mesh_remapping.py:557-594 with torch's CPU operators on the arrays of a synthetic case (matrices given instead of cameras)"""
    t = {k: torch.from_numpy(v) for k, v in case.items()}
    v_rgb, vis = t["v_rgb"], t["visible"].bool()
    acc, wacc = torch.zeros_like(v_rgb), torch.zeros_like(v_rgb[..., [0]])
    for b in range(vis.shape[0]):
        v = t["v_pos"][vis[b]]
        rgb_vis = v_rgb[vis[b]].clone()
        w_vis = torch.zeros_like(rgb_vis[..., [0]])
        homo = torch.cat([v, torch.ones_like(v[..., [0]])], -1) @ t["xform"][b].T
        clip = homo @ t["proj"][b].T
        ndc = clip[..., :2] / clip[..., [3]]
        ok = torch.logical_and(ndc > -1, ndc < 1).prod(-1).bool()
        g = ndc[ok][None, :, None]
        rgba = torch.nn.functional.grid_sample(t["images"][b][None], g, padding_mode="reflection", mode="bilinear", align_corners=False)[0, :, :, 0].T
        cw = torch.nn.functional.grid_sample(t["wmap"][b][None].permute(0, 3, 1, 2), g, padding_mode="zeros", mode="bilinear", align_corners=False)[0, :, :, 0].T
        rgb, a = rgba[:, :3], rgba[:, 3:]
        if not use_alpha:
            a = torch.ones_like(a)
        rgb_vis[ok] = rgb * a + rgb_vis[ok] * (1 - a)
        w_vis[ok] = t["weights"][b] * cw[:, :1].square().square() * (1 - cw[:, 1:])
        acc[vis[b]] = acc[vis[b]] + w_vis * rgb_vis
        wacc[vis[b]] = wacc[vis[b]] + w_vis
    return acc.numpy(), wacc.numpy()


def _grid_mesh(n):
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return np.concatenate([np.stack([a, b, c], -1), np.stack([b, d, c], -1)]).astype(np.int32)


G20_TAGS = (("p", True), ("o", False))


def g20():
    return np.load(os.path.join(ROOT, "tests", "golden", "g20_vertex_bake.npz"))


def g20_case(f, tag, perspective, mode):
    """the fixture's arrays as a projection problem; the matrices come from the PRODUCT's camera functions (texturetools/camera.py)"""
    from unitex_amd.texturetools import camera
    c2ws = torch.from_numpy(f["c2ws_" + tag])
    intr = torch.from_numpy(f["intr_" + tag]).expand(3, -1, -1)
    xform = (c2ws if mode == "ref" else camera.c2w_to_w2c(c2ws)).numpy()
    return dict(v_pos=f["verts"], visible=f["vis_" + tag], xform=xform, proj=camera.intr_to_proj(intr, perspective=perspective).numpy(), images=f["images"][:3],
                wmap=f["wmap_" + tag], v_rgb=f["v_rgb"], weights=f["weights3"])


def g20_edge(f, tag):
    g64 = weight_maps(f["cos_ray_normal_" + tag], None, 0, np.float64)["grad"]
    return np.abs(g64 - float(GRAD_THR32)) <= GRAD_EDGE
