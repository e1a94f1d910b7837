"""Restatement (TEST INFRASTRUCTURE ONLY), written for this project, of the Poisson image fusion rule of DESIGN 8 "Poisson image fusion" (csrc/image_fusion.hip:
utx_mask_morph, utx_mask_bbox, utx_image_fusion) in numpy / scipy float64, shared by tests/test_image_fusion_cpu.py and tests/test_image_fusion_gpu.py.

The rule, per image (src, dst uint8 [H,W,3], mask uint8 [H,W]):
  1. n_erode_pix > 0: grey erosion (minimum) of the mask over an n x n box, < 0: grey dilation (maximum) over |n| x |n|; the box covers the offsets
     -(n // 2) .. n - 1 - n // 2 in both axes; pixels outside the image are left out of the minimum / maximum (set for erosion, clear for dilation).
  2. R = (x1, y1, w, h): the tight bounding rectangle of mask > 0.  Empty mask, w < 3 or h < 3: the result is dst.
  3. inside R: s = src where mask > 0, else 0; m = mask / 255 eroded three times by a 3 x 3 box inside R (= the minimum over the 7 x 7 window clipped to R);
     forward differences; v = m grad(s) + (1 - m) grad(dst) with m at (x, y); f = the backward divergence of v; the unknown I on the (w-2) x (h-2) interior has
     5-point Laplacian f and equals dst on R's ring.  Solved for u = I - dst: zero boundary values, right-hand side div(m grad(s - dst)).
     Interior: clamp(round_half_even(dst + u), 0, 255); the ring and everything outside R: dst.

The exact solve: the type-I sine transform diagonalises the 5-point Laplacian with zero boundary values (solve_dst); solve_sparse is an independent direct solve
(scipy.sparse) that one CPU test holds the first against.

`mistakes` (a set of names) injects one kernel mistake each, so that the tests can show that their comparison rejects it:
  erode_twice        m eroded twice instead of three times (a 5 x 5 window)
  backward_diff      backward differences for the gradient (and the forward divergence, so that the stencil stays inside R): m is taken at the other end of each edge
  src_not_zeroed     s = src everywhere in R.  NOT observable under this rule, with any input: m(x, y) > 0 needs mask > 0 on the whole 7 x 7 window of (x, y), which
                     holds both ends of the two edges that m(x, y) weighs, so every difference of s that reaches f is a difference of src under the mask
  ring_overwritten   R's border ring takes s instead of dst
  round_half_up      floor(v + 0.5) instead of round-half-even
  one_cycle_short    one V-cycle too few: the exact correction u short by u * CONTRACTION ** (cycles - 1) (the solver starts from u = 0, so its error after k
                     cycles is modelled as u * CONTRACTION ** k)

RECORDED_D and CONTRACTION are measured on the MI355X (tools/bench_image_fusion.py); BOUND = 4 RECORDED_D is what the tests hold the float32 output to.
"""
import numpy as np

MISTAKES = ("erode_twice", "backward_diff", "src_not_zeroed", "ring_overwritten", "round_half_up", "one_cycle_short")

RECORDED_D = 0.001037      # max |float32 output - float64 oracle| in uint8 units over the GPU test's cases, measured on the MI355X
CONTRACTION = 0.053     # the worst measured error contraction per V-cycle
BOUND = 4.0 * RECORDED_D
assert BOUND <= 0.25


def default_cycles(w, h):
    """the kernel's fixed cycle count (utx_image_fusion with cycles = 0, utx_image_fusion_cycles): 4 up to max(w, h) = 512, 5 above"""
    return 4 if max(int(w), int(h)) <= 512 else 5


def morph(mask, n):
    """rule 1 on a uint8 [H,W] mask; n = 0 returns it unchanged"""
    mask = np.asarray(mask, np.uint8)
    if n == 0:
        return mask.copy()
    k, erode = abs(int(n)), n > 0
    a = k // 2
    H, W = mask.shape
    fill = 255 if erode else 0
    pad = np.full((H + k, W + k), fill, np.uint8)
    pad[a:a + H, a:a + W] = mask
    out = np.full((H, W), fill, np.uint8)
    for dy in range(k):
        for dx in range(k):
            win = pad[dy:dy + H, dx:dx + W]      # = mask[y + dy - a, x + dx - a]
            out = np.minimum(out, win) if erode else np.maximum(out, win)
    return out


def bounding_rect(mask):
    """(x1, y1, w, h) of mask > 0; (0, 0, 0, 0) for an empty mask"""
    ys, xs = np.nonzero(np.asarray(mask) > 0)
    if ys.size == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def eroded_weight(mask_r, times=3):
    """m of rule 3 on the rectangle's own mask [h,w]: mask / 255 eroded `times` times by a 3 x 3 box, pixels outside the rectangle left out"""
    m = np.asarray(mask_r, np.float64) / 255.0
    h, w = m.shape
    for _ in range(times):
        pad = np.full((h + 2, w + 2), np.inf)
        pad[1:-1, 1:-1] = m
        m = np.min([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)
    return m


def rhs(src_r, dst_r, mask_r, mistakes=()):
    """f [h-2, w-2, 3] float64 for the correction u: div(m grad(s - dst)) on the interior of the rectangle"""
    s = np.asarray(src_r, np.float64)
    if "src_not_zeroed" not in mistakes:
        s = s * (np.asarray(mask_r) > 0)[..., None]
    g = s - np.asarray(dst_r, np.float64)
    m = eroded_weight(mask_r, 2 if "erode_twice" in mistakes else 3)[..., None]
    dx = g[:, 1:] - g[:, :-1]      # dx[y, x] = g(x + 1, y) - g(x, y)
    dy = g[1:, :] - g[:-1, :]
    if "backward_diff" in mistakes:
        vx, vy = m[:, 1:] * dx, m[1:, :] * dy
    else:
        vx, vy = m[:, :-1] * dx, m[:-1, :] * dy
    return (vx[1:-1, 1:] - vx[1:-1, :-1]) + (vy[1:, 1:-1] - vy[:-1, 1:-1])


def solve_dst(f):
    """u [ny,nx,...] with u(x+1) + u(x-1) + u(y+1) + u(y-1) - 4 u = f and zero boundary values, by the type-I sine transform"""
    from scipy.fft import dstn, idstn
    f = np.asarray(f, np.float64)
    ny, nx = f.shape[:2]
    ey = 2.0 * np.cos(np.pi * np.arange(1, ny + 1) / (ny + 1)) - 2.0
    ex = 2.0 * np.cos(np.pi * np.arange(1, nx + 1) / (nx + 1)) - 2.0
    eig = (ey[:, None] + ex[None, :]).reshape((ny, nx) + (1,) * (f.ndim - 2))
    return idstn(dstn(f, type=1, axes=(0, 1)) / eig, type=1, axes=(0, 1))


def solve_sparse(f):
    """the same system by a sparse direct solve (small sizes)"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    f = np.asarray(f, np.float64)
    ny, nx = f.shape[:2]
    def lap1(n):
        return sp.diags([np.ones(n - 1), -2.0 * np.ones(n), np.ones(n - 1)], [-1, 0, 1], shape=(n, n))
    A = (sp.kron(sp.identity(ny), lap1(nx)) + sp.kron(lap1(ny), sp.identity(nx))).tocsc()
    flat = f.reshape(ny * nx, -1)
    u = np.stack([np.atleast_1d(spsolve(A, flat[:, c])) for c in range(flat.shape[1])], axis=-1)
    return u.reshape(f.shape)


def fuse(src, dst, mask, n_erode_pix=0, mistakes=()):
    """the whole rule on one image -> dict(u8 [H,W,3] uint8, f [H,W,3] float64 unrounded and unclamped (dst outside the interior), rect, interior [H,W] bool)"""
    src, dst = np.asarray(src, np.uint8), np.asarray(dst, np.uint8)
    mask = morph(mask, n_erode_pix)
    x1, y1, w, h = rect = bounding_rect(mask)
    out_f = dst.astype(np.float64)
    interior = np.zeros(mask.shape, bool)
    if w >= 3 and h >= 3:
        sl = (slice(y1, y1 + h), slice(x1, x1 + w))
        u = solve_dst(rhs(src[sl], dst[sl], mask[sl], mistakes))
        if "one_cycle_short" in mistakes:
            u = u - u * CONTRACTION ** (default_cycles(w, h) - 1)
        if "ring_overwritten" in mistakes:
            out_f[sl] = src[sl].astype(np.float64) * (mask[sl] > 0)[..., None]
        interior[y1 + 1:y1 + h - 1, x1 + 1:x1 + w - 1] = True
        out_f[y1 + 1:y1 + h - 1, x1 + 1:x1 + w - 1] = dst[y1 + 1:y1 + h - 1, x1 + 1:x1 + w - 1] + u
    rounded = np.floor(out_f + 0.5) if "round_half_up" in mistakes else np.rint(out_f)
    return dict(u8=np.clip(rounded, 0, 255).astype(np.uint8), f=out_f, rect=rect, interior=interior, mask=mask)


def excused(ref_f, bound):
    """the pixels whose rounding the bound cannot decide: the oracle's unrounded value within `bound` of a rounding tie or of a clamp edge"""
    frac = ref_f - np.floor(ref_f)
    return (np.abs(frac - 0.5) <= bound) | (np.abs(ref_f) <= bound) | (np.abs(ref_f - 255.0) <= bound)


def compare(got_u8, got_f, dst, ref, bound=None):
    """The comparison of the GPU test.  got_u8 uint8, got_f float (the unrounded output), ref = fuse(...).  Returns (problems, d, share): the list of the
    checks that fail (empty = accepted), d = max |got_f - oracle| on the interior, share = the part of the interior that the bound excuses from exact equality
    (counted from the oracle alone)."""
    bound = BOUND if bound is None else bound
    got_u8, got_f, dst = np.asarray(got_u8), np.asarray(got_f, np.float64), np.asarray(dst, np.uint8)
    inside = ref["interior"]
    problems = []
    if not np.array_equal(got_u8[~inside], dst[~inside]):
        problems.append("pixels outside the interior differ from dst")
    if not np.array_equal(got_f[~inside], dst[~inside].astype(np.float64)):
        problems.append("float pixels outside the interior differ from dst")
    if not np.array_equal(got_u8, np.clip(np.rint(got_f), 0, 255).astype(np.uint8)):
        problems.append("the uint8 output is not the half-even rounding of the float output")
    d, share = 0.0, 0.0
    if inside.any():
        rf, gf = ref["f"][inside], got_f[inside]
        d = float(np.abs(gf - rf).max())
        if d > bound:
            problems.append("max |float32 - oracle| = %.4g > %.4g" % (d, bound))
        ru, gu = ref["u8"][inside].astype(np.int64), got_u8[inside].astype(np.int64)
        if np.abs(gu - ru).max() > 1:
            problems.append("a uint8 output is more than one step from the oracle's rounding")
        ex = excused(rf, bound)
        share = float(ex.mean())
        if (gu != ru)[~ex].any():
            problems.append("%d uint8 outputs differ from the oracle away from every tie and clamp edge" % int((gu != ru)[~ex].sum()))
        if share > 2.0 * bound + 0.01:
            problems.append("excused share %.4f > %.4f" % (share, 2.0 * bound + 0.01))
    return problems, d, share


# ---- the shared inputs of the two test modules


def smooth_image(rng, H, W):
    """a seeded random uint8 image [H,W,3] smoothed once by a 3 x 3 box"""
    a = rng.integers(0, 256, size=(H + 2, W + 2, 3)).astype(np.float64)
    s = sum(a[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) / 9.0
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def step_pair(H, W):
    """the hard pair: a vertical step edge in src against a horizontal one in dst (levels away from the clamp edges)"""
    src = np.zeros((H, W, 3), np.uint8)
    dst = np.zeros((H, W, 3), np.uint8)
    src[:, W // 2:] = (230, 200, 215)
    src[:, :W // 2] = (25, 40, 30)
    dst[H // 2:] = (30, 235, 128)
    dst[:H // 2] = (220, 20, 127)
    return src, dst


def box_mask(H, W, x1, y1, w, h):
    m = np.zeros((H, W), np.uint8)
    m[y1:y1 + h, x1:x1 + w] = 255
    return m


def ellipse_mask(H, W, x1, y1, w, h):
    """an ellipse whose bounding rectangle is (x1, y1, w, h)"""
    yy, xx = np.mgrid[0:H, 0:W]
    cx, cy = x1 + (w - 1) / 2.0, y1 + (h - 1) / 2.0
    return ((((xx - cx) / (w / 2.0)) ** 2 + ((yy - cy) / (h / 2.0)) ** 2 <= 1.0) * 255).astype(np.uint8)


def _case(seed, H, W, mask, n=0, step=False):
    if step:
        src, dst = step_pair(H, W)
    else:
        rng = np.random.default_rng(seed)
        src, dst = smooth_image(rng, H, W), smooth_image(rng, H, W)
    return dict(src=src, dst=dst, mask=mask, n=n)


def edge_cases():
    """name -> dict(src, dst, mask, n): the edge shapes of the GPU test (sizes are the rectangle's w x h; its interior is two less).  Built once per process."""
    global _EDGE_CASES
    if _EDGE_CASES is not None:
        return _EDGE_CASES
    c = {}
    c["rect_3x3"] = _case(5, 12, 14, box_mask(12, 14, 5, 4, 3, 3))
    c["rect_4x4"] = _case(3, 12, 14, box_mask(12, 14, 5, 4, 4, 4))
    for k, (nx, ny) in enumerate([(31, 33), (32, 65), (33, 64), (64, 31), (65, 32)]):      # 31, 32, 33 and 64, 65 in either axis: the smoother's tile edges
        H, W = ny + 2 + 7, nx + 2 + 9
        mk = ellipse_mask if k % 2 == 0 else box_mask
        c["interior_%dx%d" % (nx, ny)] = _case(10 + k, H, W, mk(H, W, 4, 3, nx + 2, ny + 2))
    c["rect_127x61_in_160x144"] = _case(20, 144, 160, ellipse_mask(144, 160, 17, 40, 127, 61))
    c["step_pair_66x67"] = _case(21, 80, 80, ellipse_mask(80, 80, 6, 5, 66, 67), step=True)
    c["whole_image"] = _case(22, 36, 40, box_mask(36, 40, 0, 0, 40, 36))
    c["touches_left"] = _case(23, 20, 24, ellipse_mask(20, 24, 0, 4, 11, 9))
    c["touches_top"] = _case(24, 20, 24, ellipse_mask(20, 24, 5, 0, 11, 9))
    c["touches_right"] = _case(25, 20, 24, ellipse_mask(20, 24, 13, 4, 11, 9))
    c["touches_bottom"] = _case(26, 20, 24, ellipse_mask(20, 24, 5, 11, 11, 9))
    hole = box_mask(48, 56, 6, 5, 40, 36)
    hole[18:27, 20:33] = 0
    c["hole"] = _case(27, 48, 56, hole)
    c["two_blobs"] = _case(28, 48, 56, np.maximum(ellipse_mask(48, 56, 3, 4, 17, 15), ellipse_mask(48, 56, 30, 22, 21, 19)))
    c["single_row_9"] = _case(29, 20, 24, box_mask(20, 24, 6, 9, 9, 1))
    for n in (-4, -1, 3):
        c["n_erode_pix_%d" % n] = _case(30 + n, 40, 44, np.maximum(ellipse_mask(40, 44, 5, 6, 25, 21), box_mask(40, 44, 30, 2, 9, 8)), n=n)
    _EDGE_CASES = c
    return c


_EDGE_CASES = None


def scale_case():
    """1024 x 1024 with a disc mask of radius 400: the low-frequency correction that the coarse grids have to carry"""
    H = W = 1024
    rng = np.random.default_rng(99)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = (((xx - 512) ** 2 + (yy - 512) ** 2 <= 400 ** 2) * 255).astype(np.uint8)
    ramp = (xx / 8.0)[..., None] + np.array([0.0, 40.0, 90.0])
    src = np.clip(smooth_image(rng, H, W) * 0.5 + ramp, 0, 255).astype(np.uint8)
    dst = np.clip(smooth_image(rng, H, W) * 0.5 + 100.0 - (yy / 16.0)[..., None], 0, 255).astype(np.uint8)
    return dict(src=src, dst=dst, mask=mask, n=0)
