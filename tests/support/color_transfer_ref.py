"""Numpy restatements of the colour-transfer rules (DESIGN 8 "Colour transfer", unitex_amd/csrc/color_transfer.hip), shared by the CPU and GPU tests and by
tools/bench_color_transfer.py.

The OT loop, in plain sequential float32 (every product and sum rounded on its own).  new = src; per step, advect = 0 and for each batch b with d = dirs[s B + b]:
    p(x) = ((x0 d0 + x1 d1) + x2 d2) + x3 d3 over the C channels; ps = p(new), pt = p(dst)
    key(f) = bits(f) | 0x80000000 for a clear sign bit, ~bits(f) for a set one: unsigned order = the total order of the bit patterns, -0 before +0
    idS = stable argsort(key(ps)), idT = stable argsort(key(pt))      ties go to the smaller pixel index
    advect[idS[r]] = advect[idS[r]] + (pt[idT[r]] - ps[idS[r]]) * d
then new = new + advect / float32(B), a true division.  This equals the reference's numpy loop (TextureTools image/color_transfer_ot.py CTSOT with
reg_sigmaXY = 0) bit for bit wherever no two projections of a batch are equal: tests/golden/g26_color_transfer_ot.npz.

The bilateral filter, with a dtype argument (float32 follows the kernel's operation order, float64 is the yardstick): r = max(1, rint(1.5 sigma_space)) (halves
to even), the support dx^2 + dy^2 <= r^2, space weights exp(-(dx^2 + dy^2) / (2 sigma_space^2)) computed in float64 and rounded to float32 (BOTH dtypes read the
rounded table: it is an input of the kernel), colour weight exp((L1 L1) coef) with L1 = (|D0| + |D1|) + |D2| and coef = float32(-0.5 / sigma_color^2),
reflect-101 borders applied repeatedly (an axis of length 1 maps to index 0), taps row-major (dy outer, dx inner, ascending) into one running sum per channel
and one of the weights w = ws * wc: out = num / den."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "g26_color_transfer_ot.npz")
G26_CASES = ("a", "b")      # a: 37 x 29 x 3, steps 3, batch 2;  b: 16 x 9 x 4, steps 2, batch 5


# ---- OT loop
def keys(p):
    """order-preserving uint32 keys of float32 values"""
    u = np.ascontiguousarray(p, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkeys(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def project(x, d):
    """((x0 d0 + x1 d1) + x2 d2) + x3 d3, every operation rounded to float32"""
    p = x[:, 0] * d[0]
    for c in range(1, x.shape[1]):
        p = p + x[:, c] * d[c]
    return p


def ot_loop(src, dst, dirs, steps, batch_size, ties=None):
    """src, dst float32 [..., C], dirs float32 [steps * batch_size, C] -> float32 of src's shape.  ties (a list): receives per step and batch the number of
    equal neighbours among the sorted source and the sorted target projections."""
    src = np.asarray(src)
    assert src.dtype == np.float32 and np.asarray(dst).dtype == np.float32 and np.asarray(dirs).dtype == np.float32
    C = src.shape[-1]
    new = src.reshape(-1, C).copy()
    dst = np.asarray(dst).reshape(-1, C)
    B = np.float32(batch_size)
    for s in range(steps):
        advect = np.zeros_like(new)
        for b in range(batch_size):
            d = dirs[s * batch_size + b]
            ps, pt = project(new, d), project(dst, d)
            ks, kt = keys(ps), keys(pt)
            ids, idt = np.argsort(ks, kind="stable"), np.argsort(kt, kind="stable")
            if ties is not None:
                ties.append((int((np.diff(ks[ids]) == 0).sum()), int((np.diff(kt[idt]) == 0).sum())))
            a = pt[idt] - ps[ids]
            advect[ids] = advect[ids] + a[:, None] * d[None, :]
        new = new + advect / B
    return new.reshape(src.shape)


def g26():
    """the fixture: per case src, dst, dirs, steps, batch, out (the reference's own output)"""
    z = np.load(GOLDEN)
    return {n: dict(src=z[n + "_src"], dst=z[n + "_dst"], dirs=z[n + "_dirs"], steps=int(z[n + "_steps"]), batch=int(z[n + "_batch"]), out=z[n + "_out"])
            for n in G26_CASES}


# ---- bilateral filter
def bilateral_radius(sigma_space):
    return max(1, int(np.rint(1.5 * float(sigma_space))))


def space_weights(sigma_space):
    r = bilateral_radius(sigma_space)
    a = np.arange(r + 1, dtype=np.float64)
    return np.exp(-(a[:, None] ** 2 + a[None, :] ** 2) / (2.0 * float(sigma_space) ** 2)).astype(np.float32)


def reflect101(p, n):
    p = np.asarray(p)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    p = np.mod(p, period)
    return np.where(p < n, p, period - p)


def bilateral(img, sigma_color, sigma_space, dtype=np.float32):
    img = np.asarray(img)
    H, W, C = img.shape
    r = bilateral_radius(sigma_space)
    ws = space_weights(sigma_space).astype(dtype)
    coef = dtype(np.float32(-0.5 / (float(sigma_color) * float(sigma_color))))
    v = img.astype(dtype)
    ys, xs = np.arange(H), np.arange(W)
    num, den = np.zeros((H, W, C), dtype), np.zeros((H, W), dtype)
    for dy in range(-r, r + 1):
        rows = v[reflect101(ys + dy, H)]
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy > r * r:
                continue
            q = rows[:, reflect101(xs + dx, W)]
            l1 = np.abs(q[..., 0] - v[..., 0])
            for c in range(1, C):
                l1 = l1 + np.abs(q[..., c] - v[..., c])
            w = ws[abs(dy), abs(dx)] * np.exp((l1 * l1) * coef)
            num = num + w[..., None] * q
            den = den + w
    out = num / den[..., None]
    assert out.dtype == dtype
    return out


BILATERAL_SIZES = ((1, 1), (1, 7), (5, 3), (16, 16), (17, 33), (70, 50))
BILATERAL_SIGMA_SPACE = (0.5, 1.0, 3.0, 16.0)      # r = 1, 2, 4 (4.5 to even), 24
BILATERAL_SIGMA_COLOR = (0.05, 5.0)
_bil_cache = {}


def bilateral_image(H, W, C):
    """a smooth ramp plus noise in [0, 1]: both colour sigmas see close and distant neighbours"""
    rng = np.random.default_rng(1000 * H + 10 * W + C)
    y, x = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.3 * np.sin(0.37 * x + 0.21 * y)
    return (base[..., None] + rng.uniform(-0.2, 0.2, (H, W, C))).astype(np.float32)


def bilateral_case(H, W, C, sigma_color, sigma_space):
    """img, the float32 and float64 restatements, d = max |f32 - f64| and the bound 4 d; computed once"""
    key = (H, W, C, sigma_color, sigma_space)
    if key not in _bil_cache:
        img = bilateral_image(H, W, C)
        f32, f64 = bilateral(img, sigma_color, sigma_space, np.float32), bilateral(img, sigma_color, sigma_space, np.float64)
        d = float(np.abs(f32.astype(np.float64) - f64).max())
        for a in (img, f32, f64):
            a.setflags(write=False)
        _bil_cache[key] = dict(img=img, f32=f32, f64=f64, d=d, bound=4.0 * d)
    return _bil_cache[key]
