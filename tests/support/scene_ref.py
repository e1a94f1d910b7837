"""Environment renderer (TEST INFRASTRUCTURE ONLY): the fp64 numpy restatement of csrc/scene.hip, i.e. of the reference's NVDiffRendererScene
(render/nvdiffrast/renderer_scene.py) with its cube lookup replaced by this library's cube rule (oracle/pbr_ref.cube_lookup), proven in
tests/test_scene_cpu.py against the reference's own torch code (fixture G23, tests/golden/make_golden_scene.py), and the counted error bounds that
tests/test_scene_gpu.py holds the kernels to.  Inputs are the fp32 arrays the kernels get; everything after that is fp64.

u = 2^-24 is the unit roundoff of fp32: one correctly rounded operation returns r (1 + e) with |e| <= u.  The bounds are first order with every rounding taken in
the same direction; `SLACK` u is added once per bound for the second-order terms (they are below 1e-3 u for every shape the tests use).

rays_d (scene_ray, then sd_normalize3).  With n = pixel centre in NDC, a = 2 fx (exact), b = 2 cx - 1, q = n + b, p = q / a, S_i = sum_j |R_ij| |p_j|:
  n = ((x + .5) / W) 2 - 1      the division 1 u of a value < 1, doubled, the subtraction 1 u of a value < 1                       dn  <= 3 u
  b                             the doubling is exact, the subtraction rounds                                                    db  <= u |b|
  q = n + b                                                                                                                      dq  <= dn + db + u |q|
  p = q / a                                                                                                                      dp  <= dq / |a| + u |p|      (p.z = -1 exact)
  w_i = ((R_i0 p.x + R_i1 p.y) + R_i2 p.z) + t_i;  d_i = w_i - t_i:  three products and two sums of magnitude <= S_i (4 u S_i: R_i2 * -1 is exact), the sum
        with t of magnitude <= S_i + |t_i|, the difference of magnitude <= S_i                                                   dd_i <= sum_j |R_ij| dp_j + u (6 S_i + |t_i|)
  normalise: the direction moves by at most |dd| / |d| and the length by the same, 5 u for the dot (3), the square root and the divide  drays <= 2 |dd|_2 / |d|_2 + 5 u

uv = (atan2(dx, -dz) / 2pi + .5, acos(clamp(dy)) / pi) with the direction good to e (per component; a vector of length <= sqrt(3) e):
  phi    moves by asin(min(1, sqrt(2) e / rho)), rho = sqrt(dx^2 + dz^2): the conditioning of atan2 at the poles (any angle once sqrt(2) e >= rho); atan2f itself
         is good to 6 ulp (OpenCL full profile, which the device's math library meets), 12 u |phi|; the constant (float)(2 pi) 1 u, the divide 1 u, + .5 1 u of a
         value <= 1.  u is compared on the circle (0 and 1 are the same column: phi = -pi and phi = +pi).
  theta  moves by max |acos(clamp(dy +- e)) - acos(dy)|, evaluated, not linearised: it grows as 1 / sqrt(1 - dy^2) and is sqrt(2 e) at a pole;
         acosf is good to 4 ulp, 8 u theta; the constant 1 u, the divide 1 u.

lookups at the kernel's OWN fp32 rays_d / uv (so no direction error times texel contrast), A = max |texel|, D = max texel - min texel (for grid_sample, whose
padding is zero, D = max(max texel, 0) - min(min texel, 0)):
  cube rule        5 ulp(A) for the three a + f (b - a) blends and the corner mean (tests/test_pbr_gpu.py); the face coordinate f = c / m 1 u, f + 1 2 u, times
                   N / 2, - .5: t is good to 3.5 u N, so is the fraction, per axis, times D; a fraction that snaps to a texel centre on one side only (rule 2)
                   jumps by <= N 2^-21 = 8 u N, per axis, times D                                                                   5 ulp(A) + 23 u N D
  wrap-linear      x = tu W - .5 is good to 2 u W (y: 2 u H), times D; t00 (1 - fx) + t01 fx: 3 u A per level, two levels       (2 W + 2 H) u D + 6 u A
  grid_sample      ix = ((g + 1) W - 1) / 2 is good to 3 u W (iy: 3 u H), times D; the four weights (1 - tx)(1 - ty) 3 u each, the products 1 u, three sums 3 u
                                                                                                                                    (3 W + 3 H) u D + 7 u A
bake: uv of view m (scene_texel_dir rounds the fp64 direction once: u per component; row4 = ((m0 x + m1 y) + m2 z) + m3 w, T_i = sum_j |m_ij| |v_j|):
  cam_i  <= sum_{j<3} |w2c_ij| u + 4 u T_i (cam_3 is exactly 1);  clip_k <= sum_i |P_ki| dcam_i + 4 u T_k;  uv = clip.xy / clip.w: (dclip_k + |uv| dclip_w) / |clip.w| + u |uv|
  the panorama: mean of cnt samples, each good to the grid_sample bound; cnt - 1 sums of magnitude <= cnt A and the divide: + (cnt + 1) u A; the clamp is a contraction."""
import os

import numpy as np

from oracle import pbr_ref as PC

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
F32, F64 = np.float32, np.float64
U = 2.0 ** -24
SLACK = 1.0
# the reference's own fp32 rounding against this restatement on G23, measured on the CPU (tests/test_scene_cpu.py prints each and holds it with a factor 2;
# DESIGN 8): maximum absolute differences; bake_uv relative to max(1, |uv|) over every (view, texel), bake_uv_inside absolute over the texels inside a view
REF_ROUNDING = dict(rays=1.12e-7, uv=7.82e-8, texel_dir=2.38e-7, cubemap_to_latlong=4.88e-7, bake_uv=1.26e-4, bake_uv_inside=5.09e-7, bake=3.12e-6,
                    bake_at_own_uv=4.13e-7)
_cache = {}


def load_g23():
    if "g23" not in _cache:
        _cache["g23"] = dict(np.load(os.path.join(GOLD, "g23_scene.npz"), allow_pickle=False))
    return _cache["g23"]


def ulp(x):
    return float(np.spacing(F32(np.abs(x).max())))


# ---------------------------------------------------------------------------------------------------------------- perspective_rendering
def _intr(intrinsics, B):
    k = np.asarray(intrinsics, F64)
    return np.broadcast_to(k, (B, 3, 3))


def rays(c2ws, intrinsics, H, W):
    """(rays_o [B,H,W,3], rays_d [B,H,W,3] fp64, bound on a fp32 rays_d [B,H,W])"""
    c2ws = np.asarray(c2ws, F64)
    B = c2ws.shape[0]
    k = _intr(intrinsics, B)
    nx = ((np.arange(W) + 0.5) / W) * 2.0 - 1.0
    ny = ((np.arange(H) + 0.5) / H) * 2.0 - 1.0
    a = np.stack([2 * k[:, 0, 0], 2 * k[:, 1, 1]], -1)[:, None, None, :]                      # [B,1,1,2]
    b = np.stack([2 * k[:, 0, 2] - 1, 2 * k[:, 1, 2] - 1], -1)[:, None, None, :]
    n = np.stack(np.broadcast_arrays(nx[None, :], ny[:, None]), -1)[None]                     # [1,H,W,2]
    q = np.concatenate([n[..., :1] + b[..., :1], b[..., 1:] - n[..., 1:]], -1)
    p2 = q / a
    p = np.concatenate([p2, -np.ones_like(p2[..., :1])], -1)                                   # [B,H,W,3]
    R, t = c2ws[:, None, None, :3, :3], c2ws[:, None, None, :3, 3]
    d = ((R * p[..., None, :]).sum(-1) + t) - t
    length = np.linalg.norm(d, axis=-1, keepdims=True)
    rd = d / np.maximum(length, 1e-12)
    dq = 3 * U + U * np.abs(b) + U * np.abs(q)
    dp = np.concatenate([dq / np.abs(a) + U * np.abs(p2), np.zeros_like(p2[..., :1])], -1)
    S = (np.abs(R) * np.abs(p[..., None, :])).sum(-1)
    dd = (np.abs(R) * dp[..., None, :]).sum(-1) + U * (6 * S + np.abs(t))
    bound = 2 * np.linalg.norm(dd, axis=-1) / length[..., 0] + (5 + SLACK) * U
    ro = np.broadcast_to(np.asarray(c2ws, F64)[:, None, None, :3, 3], rd.shape)
    return ro, rd, bound


def dir_uv(d):
    d = np.asarray(d, F64)
    return np.stack([np.arctan2(d[..., 0], -d[..., 2]) / (2 * np.pi) + 0.5, np.arccos(np.clip(d[..., 1], -1, 1)) / np.pi], -1)


def uv_bound(d, e):
    """bound [...,2] on the fp32 uv of a direction known to e per component around the fp64 direction d (module docstring)"""
    d, e = np.asarray(d, F64), np.asarray(e, F64)
    rho = np.hypot(d[..., 0], d[..., 2])
    phi, theta = np.arctan2(d[..., 0], -d[..., 2]), np.arccos(np.clip(d[..., 1], -1, 1))
    dphi = np.where(np.sqrt(2) * e >= rho, np.pi, np.arcsin(np.minimum(1.0, np.sqrt(2) * e / np.maximum(rho, 1e-300))))
    du = (dphi + 12 * U * np.abs(phi)) / (2 * np.pi) + 2 * U * np.abs(phi) / (2 * np.pi) + (1 + SLACK) * U
    dth = np.maximum(np.abs(np.arccos(np.clip(d[..., 1] + e, -1, 1)) - theta), np.abs(np.arccos(np.clip(d[..., 1] - e, -1, 1)) - theta))
    dv = (dth + 8 * U * theta) / np.pi + (2 + SLACK) * U * theta / np.pi
    return np.stack([du, dv], -1)


def circle_diff(a, b):
    """|a - b| on the unit circle (the panorama's u: 0 and 1 are the same column)"""
    x = np.abs(np.asarray(a, F64) - np.asarray(b, F64))
    return np.minimum(x, np.abs(1.0 - x))


def wrap_linear(tex, uv):
    """dr.texture(filter 'linear', wrap in both axes) of tex [Hi,Wi,C] at uv [...,2], fp64"""
    tex, uv = np.asarray(tex, F64), np.asarray(uv, F64)
    Hi, Wi = tex.shape[:2]
    x, y = uv[..., 0] * Wi - 0.5, uv[..., 1] * Hi - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    ix = lambda t: np.mod(t.astype(np.int64), Wi)
    iy = lambda t: np.mod(t.astype(np.int64), Hi)
    top = tex[iy(y0), ix(x0)] * (1 - fx) + tex[iy(y0), ix(x0 + 1)] * fx
    bot = tex[iy(y0 + 1), ix(x0)] * (1 - fx) + tex[iy(y0 + 1), ix(x0 + 1)] * fx
    return top * (1 - fy) + bot * fy


def cube_bound(cube):
    cube = np.asarray(cube, F64)
    return 5 * ulp(cube) + (23 + SLACK) * U * cube.shape[1] * (cube.max() - cube.min())


def wrap_bound(tex):
    tex = np.asarray(tex, F64)
    return (2 * tex.shape[0] + 2 * tex.shape[1] + SLACK) * U * (tex.max() - tex.min()) + 6 * U * np.abs(tex).max()


def grid_bound(img):
    """img [...,H,W,C]"""
    img = np.asarray(img, F64)
    H, W = img.shape[-3], img.shape[-2]
    return (3 * H + 3 * W + SLACK) * U * (max(img.max(), 0.0) - min(img.min(), 0.0)) + 7 * U * np.abs(img).max()


# ---------------------------------------------------------------------------------------------------------------- the panorama's grid
def texel_dirs(Ht, Wt):
    gx, gy = 2.0 * ((np.arange(Wt) + 0.5) / Wt) - 1.0, 2.0 * ((np.arange(Ht) + 0.5) / Ht) - 1.0
    psi, theta = (gx * np.pi)[None, :], (gy * (np.pi / 2) + np.pi / 2)[:, None]
    return np.stack(np.broadcast_arrays(np.sin(theta) * np.sin(psi), np.cos(theta), -np.sin(theta) * np.cos(psi)), -1)


def cubemap_to_latlong(cube, Ht, Wt):
    """the cube rule at the grid's directions, rounded once to fp32 as the kernel rounds them"""
    return PC.cube_lookup(cube, texel_dirs(Ht, Wt).astype(F32))


def cubemap_to_latlong_bound(cube):
    """cube_bound plus one fp32 ulp of the direction (the device's fp64 sin / cos may round the other way): K u, K = 2 * 2 sqrt(3) * (N / 2) * D (oracle/pbr_ref.py)"""
    cube = np.asarray(cube, F64)
    return cube_bound(cube) + 2 * 2 * np.sqrt(3.0) * (cube.shape[1] / 2) * (cube.max() - cube.min()) * 2 * U


# ---------------------------------------------------------------------------------------------------------------- the bake
def _row4(m, v):
    """m [M,1,1,4,4], v [...,4] -> (m v [...,4], sum_j |m_ij| |v_j|)"""
    return (m * v[..., None, :]).sum(-1), (np.abs(m) * np.abs(v[..., None, :])).sum(-1)


def bake_project(w2cs, projs, Ht, Wt):
    """-> uv [M,Ht,Wt,2], depth [M,Ht,Wt], alpha [M,Ht,Wt] bool, bound on a fp32 uv [M,Ht,Wt,2], bound on a fp32 depth [M,Ht,Wt]"""
    w2c = np.asarray(w2cs, F64)[:, None, None]
    P = np.broadcast_to(np.asarray(projs, F64), (w2c.shape[0], 4, 4))[:, None, None]      # one shared projection or one per view
    rd = texel_dirs(Ht, Wt)
    p = np.concatenate([rd, np.ones_like(rd[..., :1])], -1)[None]
    cam, Tc = _row4(w2c, p)
    dcam = np.abs(w2c[..., :3]).sum(-1) * U + 4 * U * Tc
    dcam[..., 3] = np.where((np.asarray(w2cs, F64)[:, 3] == [0, 0, 0, 1]).all(-1)[:, None, None], 0.0, dcam[..., 3])
    clip, Tp = _row4(P, cam)
    dclip = (np.abs(P) * dcam[..., None, :]).sum(-1) + 4 * U * Tp
    depth = clip[..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = clip[..., :2] / depth[..., None]
        bound = (dclip[..., :2] + np.abs(uv) * dclip[..., 3:4]) / np.abs(depth[..., None]) + (1 + SLACK) * U * np.abs(uv)
    alpha = (uv >= -1).all(-1) & (uv <= 1).all(-1) & (depth > 0)
    return uv, depth, alpha, bound, dclip[..., 3]


def bake_margin_ok(uv, depth, bound, dbound):
    """every texel's mask is decided with room to spare: no uv within its bound of +-1, no depth within its bound of 0 (then fp32 and fp64 agree on the mask)"""
    with np.errstate(invalid="ignore"):
        near_edge = (np.abs(np.abs(uv) - 1.0) <= bound) & (depth > 0)[..., None]
    return not near_edge.any() and not (np.abs(depth) <= dbound).any()


def grid_sample(img, uv):
    """F.grid_sample(bilinear, zeros, align_corners=False) of img [M,H,W,C] at uv [M,...,2], fp64; non-finite coordinates sample 0"""
    img, uv = np.asarray(img, F64), np.asarray(uv, F64)
    M, H, W, _ = img.shape
    ok = np.isfinite(uv).all(-1)
    g = np.where(ok[..., None], uv, -3.0)
    ix, iy = ((g[..., 0] + 1) * W - 1) * 0.5, ((g[..., 1] + 1) * H - 1) * 0.5
    x0, y0 = np.floor(ix), np.floor(iy)
    tx, ty = ix - x0, iy - y0
    m = np.arange(M).reshape((M,) + (1,) * (uv.ndim - 2))
    out = 0.0
    for dy, dx, w in ((0, 0, (1 - tx) * (1 - ty)), (0, 1, tx * (1 - ty)), (1, 0, (1 - tx) * ty), (1, 1, tx * ty)):
        x, y = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        out = out + np.where(inside[..., None], img[m, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0.0) * w[..., None]
    return np.where(ok[..., None], out, 0.0)


def bake(images, uv, alpha):
    """(the baked panorama [Ht,Wt,C], the number of views that see each texel [Ht,Wt]) from the views' uv [M,Ht,Wt,2] and masks [M,Ht,Wt]"""
    a = np.asarray(alpha, F64).reshape(np.asarray(uv).shape[:-1])
    s = (grid_sample(images, uv) * a[..., None]).sum(0)
    cnt = a.sum(0)
    out = np.where(cnt[..., None] > 0, s / np.maximum(cnt, 1.0)[..., None], 0.0)
    return np.clip(out, 0.0, 1.0), cnt


def bake_bound(images, cnt):
    return grid_bound(images) + (np.asarray(cnt, F64) + 1) * U * np.abs(np.asarray(images, F64)).max()
