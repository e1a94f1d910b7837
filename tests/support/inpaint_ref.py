"""Numpy restatement of the Telea inpainting rule (DESIGN 8 "Telea inpainting", unitex_amd/csrc/inpaint.hip), with a dtype argument: float32 follows the kernel's
operation order, float64 is the yardstick.  Also the brute-force integer distance, the shared case list of the CPU and GPU tests, and the one comparison both use.

The rule.  D2(p): the exact squared Euclidean distance (integer) of a hole pixel to the nearest in-image pixel outside the hole, 0 outside the hole, NONE
everywhere when the whole image is a hole (nothing is filled then).  T = sqrt(dtype(D2)).  For a hole pixel p and radius eps:
    A(p) = { q in the image : |q - p|^2 <= eps^2 and D2(q) < D2(p) }        strict, on integers; a pixel outside the hole has D2 = 0
Per channel, q enumerated ROW-MAJOR over the (2 eps + 1)^2 window (dy outer, dx inner, ascending), r = p - q = (rx, ry) = (-dx, -dy):
    len2 = dtype(rx rx + ry ry); len = sqrt(len2); dst = 1 / (len2 * len); lev = 1 / (1 + |T(q) - T(p)|)
    dir = max(|rx * gTx + ry * gTy|, 1e-6); w = (dst * lev) * dir
    val = I(q) + (gIx * rx + gIy * ry); num = num + w * val; den = den + w   (ONE running sum each, in the enumeration order; a pixel outside A(p) adds nothing)
    v = num / den
gT(p): (T(+1) - T(-1)) * 0.5 where both neighbours are in the image, T(+1) - T(0) / T(0) - T(-1) at the image border, 0 on an axis of length 1.
gI(q) per axis over the neighbours n of q in the image with D2(n) < D2(p): (I(+1) - I(-1)) * 0.5 with both, I(+1) - I(0) / I(0) - I(-1) with one, 0 with none.
The working image stays in dtype; the output is clip(v, 0, 255) rounded half to even once at the end.  Everything p reads has a smaller D2: any schedule that
honours that order gives the same bits.  Two are here: by ascending D2 ('sorted') and the kernel's sweeps ('sweep': p computes once every pixel of its read
set -- the disc and the 4-neighbours of the disc's pixels -- with a smaller D2 is done), which also counts the sweeps."""
import numpy as np

NONE = 2 ** 31 - 1
RADIUS_MAX = 8


# ---- distance
def distance_brute(hole, metric="euclid"):
    """min over every pixel outside the hole of |q - p|^2, by enumeration (int64 inside, int32 out)"""
    hole = np.asarray(hole) != 0
    H, W = hole.shape
    out = np.zeros((H, W), np.int64)
    ky, kx = np.nonzero(~hole)
    hy, hx = np.nonzero(hole)
    if len(hy) == 0:
        return out.astype(np.int32)
    if len(ky) == 0:
        return np.full((H, W), NONE, np.int32)
    for s in range(0, len(hy), 512):
        dy = np.abs(hy[s:s + 512, None].astype(np.int64) - ky[None])
        dx = np.abs(hx[s:s + 512, None].astype(np.int64) - kx[None])
        d = dy * dy + dx * dx if metric == "euclid" else (dy + dx) ** 2
        out[hy[s:s + 512], hx[s:s + 512]] = d.min(1)
    return out.astype(np.int32)


def distance(hole):
    """the kernel's two passes: g = the vertical distance to the nearest pixel outside the hole in the column, then min over the row of dx^2 + g^2"""
    hole = np.asarray(hole) != 0
    H, W = hole.shape
    INF = 1 << 30
    g = np.full((H, W), INF, np.int64)
    d = np.full(W, INF, np.int64)
    for y in range(H):
        d = np.where(~hole[y], 0, np.where(d < INF, d + 1, d))
        g[y] = d
    d = np.full(W, INF, np.int64)
    for y in range(H - 1, -1, -1):
        d = np.where(~hole[y], 0, np.where(d < INF, d + 1, d))
        g[y] = np.minimum(g[y], d)
    xs = np.arange(W)
    dx2 = (xs[:, None] - xs[None]) ** 2      # [x, x']
    out = np.empty((H, W), np.int64)
    for y in range(H):
        cand = np.where(g[y][None] < INF, dx2 + g[y][None] ** 2, NONE)
        out[y] = cand.min(1)
    return out.astype(np.int32)


# ---- the value
def window_offsets(eps, window="disc"):
    """(dy, dx) row-major over the window, the centre left out"""
    o = [(dy, dx) for dy in range(-eps, eps + 1) for dx in range(-eps, eps + 1) if (dy or dx) and (window == "square" or dy * dy + dx * dx <= eps * eps)]
    return np.array(o, np.int64).reshape(-1, 2)


def read_set_offsets(eps):
    """the disc and the 4-neighbours of the disc's pixels"""
    disc = {(dy, dx) for dy in range(-eps, eps + 1) for dx in range(-eps, eps + 1) if dy * dy + dx * dx <= eps * eps}
    s = set(disc)
    for dy, dx in disc:
        s |= {(dy + 1, dx), (dy - 1, dx), (dy, dx + 1), (dy, dx - 1)}
    s.discard((0, 0))
    return np.array(sorted(s), np.int64)


def grad_T(T):
    H, W = T.shape
    gx, gy = np.zeros_like(T), np.zeros_like(T)
    if W > 1:
        gx[:, 1:-1] = (T[:, 2:] - T[:, :-2]) * 0.5
        gx[:, 0] = T[:, 1] - T[:, 0]
        gx[:, -1] = T[:, -1] - T[:, -2]
    if H > 1:
        gy[1:-1] = (T[2:] - T[:-2]) * 0.5
        gy[0] = T[1] - T[0]
        gy[-1] = T[-1] - T[-2]
    return gx, gy


class _State:
    def __init__(self, img, D2, eps, dtype):
        H, W, C = img.shape
        self.h = h = eps + 1
        self.I = np.zeros((H + 2 * h, W + 2 * h, C), dtype)
        self.I[h:h + H, h:h + W] = img.astype(dtype)
        self.D2 = np.full((H + 2 * h, W + 2 * h), NONE, np.int64)
        self.D2[h:h + H, h:h + W] = D2
        T = np.sqrt(D2.astype(dtype))
        self.T = np.zeros((H + 2 * h, W + 2 * h), dtype)
        self.T[h:h + H, h:h + W] = T
        self.gTx, self.gTy = grad_T(T)


def _values(st, py, px, eps, dtype, strict=True, gradient=True, window="disc", swap_r=False):
    """the rule for the pixels (py, px) (unpadded coordinates) from the state's working image -> [n, C]"""
    h = st.h
    off = window_offsets(eps, window)
    oy, ox = off[:, 0], off[:, 1]
    qy, qx = py[:, None] + h + oy[None], px[:, None] + h + ox[None]
    D2p = st.D2[py + h, px + h][:, None]
    less = (lambda a: a < D2p) if strict else (lambda a: a <= D2p)
    av = less(st.D2[qy, qx])
    rx, ry = (-ox).astype(dtype), (-oy).astype(dtype)
    if swap_r:
        rx, ry = ry, rx
    len2 = (ox * ox + oy * oy).astype(dtype)
    dst = 1.0 / (len2 * np.sqrt(len2))
    lev = 1.0 / (1.0 + np.abs(st.T[qy, qx] - st.T[py + h, px + h][:, None]))
    dirw = np.maximum(np.abs(rx[None] * st.gTx[py, px][:, None] + ry[None] * st.gTy[py, px][:, None]), dtype(1e-6))
    w = (dst[None] * lev) * dirw
    Iq = st.I[qy, qx]
    if gradient:
        def axis(ay, ax):
            a, b = less(st.D2[qy + ay, qx + ax])[..., None], less(st.D2[qy - ay, qx - ax])[..., None]
            Ip, Im = st.I[qy + ay, qx + ax], st.I[qy - ay, qx - ax]
            return np.where(a & b, (Ip - Im) * 0.5, np.where(a, Ip - Iq, np.where(b, Iq - Im, dtype(0))))
        val = Iq + (axis(0, 1) * rx[None, :, None] + axis(1, 0) * ry[None, :, None])
    else:
        val = Iq
    n, C = len(py), Iq.shape[2]
    num, den = np.zeros((n, C), dtype), np.zeros(n, dtype)
    for k in range(len(off)):      # the summation order: one running sum, row-major over the window
        num = num + np.where(av[:, k, None], w[:, k, None] * val[:, k], dtype(0))
        den = den + np.where(av[:, k], w[:, k], dtype(0))
    assert num.dtype == dtype and den.dtype == dtype
    return num / den[:, None]


def round_u8(v, rounding="even"):
    c = np.clip(v, 0, 255)
    return (np.rint(c) if rounding == "even" else np.floor(c + 0.5)).astype(np.uint8)


def telea(img, hole, eps=1, dtype=np.float64, schedule="sorted", metric="euclid", rounding="even", **mutation):
    """img uint8 [H,W,C], hole [H,W] (non-zero: fill) -> (uint8 [H,W,C], the working image in dtype unrounded and unclamped, sweeps or levels)"""
    img, hole = np.asarray(img), np.asarray(hole) != 0
    eps = max(int(eps), 1)
    assert eps <= RADIUS_MAX and img.ndim == 3 and 1 <= img.shape[2] <= 4 and hole.shape == img.shape[:2]
    if hole.size == 0 or not hole.any() or hole.all():
        return img.copy(), img.astype(dtype), 0
    D2 = distance(hole) if metric == "euclid" else distance_brute(hole, metric)
    st = _State(img, D2, eps, dtype)
    H, W = hole.shape
    h = st.h
    steps = 0
    if schedule == "sorted":
        hy, hx = np.nonzero(hole)
        d = D2[hy, hx]
        for lvl in np.unique(d):
            sel = d == lvl
            v = _values(st, hy[sel], hx[sel], eps, dtype, **mutation)
            st.I[hy[sel] + h, hx[sel] + h] = v
            steps += 1
    else:
        assert schedule == "sweep" and not mutation
        done = np.zeros((H + 2 * h, W + 2 * h), bool)
        done[h:h + H, h:h + W] = ~hole
        rs = read_set_offsets(eps)
        while True:
            py, px = np.nonzero(~done[h:h + H, h:h + W])
            if len(py) == 0:
                break
            ny, nx = py[:, None] + h + rs[None, :, 0], px[:, None] + h + rs[None, :, 1]
            ready = ~((st.D2[ny, nx] < D2[py, px][:, None]) & ~done[ny, nx]).any(1)
            assert ready.any()
            py, px = py[ready], px[ready]
            v = _values(st, py, px, eps, dtype)      # from the previous sweep's state: nothing computed in this sweep is read
            st.I[py + h, px + h] = v
            done[py + h, px + h] = True
            steps += 1
    out_f = st.I[h:h + H, h:h + W].copy()
    return round_u8(out_f, rounding), out_f, steps


# ---- the cases and the comparison shared by the CPU and GPU tests
def _image(rng, H, W, C):
    """a smooth field with a little noise, in uint8: what a texture atlas holds"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.empty((H, W, C))
    for c in range(C):
        a, b, ph = rng.uniform(0.05, 0.25, 3)
        img[..., c] = 128 + 90 * np.sin(a * x + ph * 7) * np.cos(b * y + c) + rng.uniform(-6, 6, (H, W))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def slanted_hole():
    """a 96 x 40 hole under a boundary of slope 1/8 in a 56 x 112 image: the distance changes by less than one per pixel along the boundary, so the dependency
    chain runs sideways and is longer than the hole is deep"""
    hole = np.zeros((56, 112), np.uint8)
    for x in range(8, 104):
        y0 = 4 + (x - 8) // 8
        hole[y0:y0 + 40, x] = 1
    return hole


_CASES, _REFERENCE = [], {}


def _reference_of(img, hole, eps):
    u64, f64, _ = telea(img, hole, eps, np.float64)
    u32, f32, _ = telea(img, hole, eps, np.float32)
    d = float(np.abs(f32.astype(np.float64) - f64).max())
    return dict(img=img, hole=hole, eps=eps, u64=u64, f64=f64, u32=u32, f32=f32, d=d, bound=4.0 * d)


def cases():
    """(name, img uint8 [H,W,C], hole uint8 [H,W], eps): images 1x1, 1x9, 9x1, 5x7, 33x31, 64x65 (they straddle the 16 x 16 LDS tiles and the waves) and the
    slanted hole's 56x112; radii 1, 2, 3, 8; C = 1, 3, 4.  Built once per process, with each case's reference.  A one-pixel hole between integers lands on a
    rounding tie about every other time (1x9: v = (2 L - L' + 2 R - R') / 2), so an image is drawn again, from the same seeded stream, until the share of the
    hole's values that the float64 restatement puts within the case's bound of a tie or a clamp edge is under the cap of 2 x bound + 1 %."""
    if _CASES:
        return list(_CASES)
    rng = np.random.default_rng(20041)

    def add(name, H, W, C, hole, eps):
        hole = np.ascontiguousarray(hole, dtype=np.uint8)
        for _ in range(4000):
            ref = _reference_of(_image(rng, H, W, C), hole, eps)
            if excused_share(ref["f64"], hole, ref["bound"]) <= 2 * ref["bound"] + 0.01:
                break
        else:
            raise AssertionError("no image under the cap for " + name)
        _CASES.append((name, ref["img"], hole, eps))
        _REFERENCE[name] = ref

    z = lambda H, W: np.zeros((H, W), np.uint8)
    add("1x1 everything", 1, 1, 1, np.ones((1, 1)), 1)
    add("1x1 nothing", 1, 1, 3, z(1, 1), 2)
    m = z(1, 9); m[0, 4] = 1
    add("1x9 single pixel", 1, 9, 3, m, 1)
    m = z(1, 9); m[0, :3] = 1
    add("1x9 at the border, window wider than the image", 1, 9, 1, m, 8)
    m = np.ones((9, 1)); m[6, 0] = 0
    add("9x1 everything except one pixel", 9, 1, 4, m, 2)
    m = np.ones((5, 7)); m[1:4, 1:6] = 0
    add("5x7 ring on every border and corner", 5, 7, 3, m, 3)
    m = z(5, 7); m[0, 0] = 1; m[4, 6] = 1; m[2, 3] = 1
    add("5x7 corners and a single pixel", 5, 7, 1, m, 1)
    m = z(33, 31); m[10:15, 5:10] = 1; m[10:15, 12:17] = 1; m[20:26, 3:9] = 1; m[27:32, 3:9] = 1
    add("33x31 two holes closer than 2 eps, eps 2", 33, 31, 1, m, 2)
    add("33x31 two holes closer than 2 eps, eps 3", 33, 31, 3, m, 3)
    m = z(33, 31); m[8:22, 9:25] = 1; m[0:5, 26:31] = 1; m[30:33, 0:4] = 1
    add("33x31 block across the tiles, corners, eps 8", 33, 31, 3, m, 8)
    m = (rng.uniform(0, 1, (33, 31)) < 0.35).astype(np.uint8)
    add("33x31 scattered, eps 8", 33, 31, 4, m, 8)
    m = z(64, 65); m[16, 16] = 1; m[15, 47] = 1; m[63, 64] = 1; m[0, 32] = 1
    add("64x65 single pixels at the tile edges", 64, 65, 4, m, 1)
    m = np.ones((64, 65)); m[40, 23] = 0
    add("64x65 everything except one pixel", 64, 65, 3, m, 1)
    add("64x65 everything", 64, 65, 3, np.ones((64, 65)), 2)
    add("64x65 nothing", 64, 65, 1, z(64, 65), 3)
    m = z(64, 65); m[:, 60:] = 1; m[58:, :] = 1; m[5:30, 0:3] = 1; m[0:2, 10:50] = 1
    add("64x65 bands on every border", 64, 65, 3, m, 2)
    add("slanted 96x40 hole, eps 1", 56, 112, 3, slanted_hole(), 1)
    add("slanted 96x40 hole, eps 3", 56, 112, 1, slanted_hole(), 3)
    return list(_CASES)


def reference(name):
    """the float64 restatement of a case of cases(), the float32 one, d = max |float32 - float64| in uint8 steps before rounding, and the case's bound 4 d --
    the margin the Poisson tests gave a different contraction and summation tree on the device.  Computed once per process and shared."""
    cases()
    return _REFERENCE[name]


def excused(ref64, bound):
    """where the float64 value lies within `bound` (uint8 steps) of a rounding tie or of a clamp edge: a value there may round either way"""
    frac = ref64 - np.floor(ref64)
    return (np.abs(frac - 0.5) <= bound) | (np.abs(ref64) <= bound) | (np.abs(ref64 - 255.0) <= bound)


def excused_share(ref64, hole, bound):
    """the share of the hole's values the comparison excuses, counted from the float64 restatement alone"""
    hole = np.asarray(hole) != 0
    return float(excused(ref64, bound)[hole].mean()) if hole.any() else 0.0


def compare(got_u8, got_f, ref64, hole, bound):
    """the comparison of the GPU test, also run on the CPU against wrong variants of the rule.  Returns a list of complaints, empty when all three hold:
    the float output within `bound` uint8 steps of the float64 restatement; the uint8 output the half-even rounding of the clamped float output; the uint8
    output equal to the rounded float64 value except where that is excused.  (The cap on the excused share is asserted on the restatement alone.)"""
    bad = []
    got_f = np.asarray(got_f, np.float64)
    d = np.abs(got_f - ref64).max() if ref64.size else 0.0
    if not d <= bound:
        bad.append("float output off by %.3g uint8 steps, bound %.3g" % (d, bound))
    if not (np.asarray(got_u8) == np.rint(np.clip(got_f, 0, 255)).astype(np.uint8)).all():
        bad.append("uint8 output is not the half-even rounding of the float output")
    wrong = (np.asarray(got_u8) != round_u8(ref64)) & ~excused(ref64, bound)
    if wrong.any():
        bad.append("%d uint8 values differ from the rounded float64 restatement away from every tie and clamp edge" % int(wrong.sum()))
    return bad
